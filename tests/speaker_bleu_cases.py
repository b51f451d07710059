"""The g16 fixture (tests/golden/g16_speaker_bleu.json.gz, written by tests/golden/make_golden_bleu.py) as test
cases: the 260 paths of R2R_sub_val_seen with their instruction texts, hypothesis sets with the numbers the
reference's eval_speaker.SpeakerEvaluation gave for them, and hand-made multi_bleu cases.  Shared by the generator
(which builds the result dictionaries it feeds the reference with `build_results`) and the tests (which build the
same dictionaries for the package)."""
import gzip
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, 'tests', 'golden', 'g16_speaker_bleu.json.gz')

_cache = {}


def load():
    if 'fx' not in _cache:
        with gzip.open(PATH, 'rt') as f:
            _cache['fx'] = json.load(f)
    return _cache['fx']


def digest(tokens):
    return hashlib.sha1('\x1f'.join(tokens).encode('utf-8')).hexdigest()[:12]


def build_results(items, case):
    """The results dictionary of a hypothesis set: one entry per instruction id of every path ('<path_id>_<j>' for
    every instruction the item has: ids an evaluator does not know are for it to ignore), all of a path with the same
    words and score -- in file order, or reversed -- except the ids `overrides` names."""
    ids = [(it['path_id'], j) for it in items for j in range(len(it['instructions']))]
    if case['order'] == 'reversed':
        ids.reverse()
    over = {o[0]: o for o in case.get('overrides', [])}
    results = {}
    for pid, j in ids:
        iid = '%d_%d' % (pid, j)
        if iid in over:
            words, score = over[iid][1], over[iid][2]
        else:
            words = case['hyps'][str(pid)]
            score = case['scores'][str(pid)] if case.get('scores') else None
        results[iid] = {'instr_id': iid, 'words': list(words)}
        if score is not None:
            results[iid]['score'] = score
    return results
