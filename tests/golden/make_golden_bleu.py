#!/usr/bin/env python3
"""G16: the reference's speaker evaluation pinned (tasks/R2R/eval_speaker.py, tasks/R2R/bleu.py and the perl script
bleu.py runs) -- BUILD container only (needs the reference tree and perl).

The reference's `eval_speaker.SpeakerEvaluation` and `bleu.multi_bleu` are imported from the reference tree and run
there (their loaders and the script's path are relative to it) on the split it ships, R2R_sub_val_seen.json: 260
paths, 258 with three instructions and 2 with four.  Nothing of the simulator is touched (eval_speaker imports utils
and bleu only).

Writes tests/golden/g16_speaker_bleu.json.gz (data only: inputs and the reference's outputs)
  items        path_id, scan, instructions (text) of the 260 paths, in file order
  vocab        the words of train_vocab.txt (what a speaker over this split generates from)
  tokens       per instruction a digest of utils.Tokenizer.split_sentence's tokens; in full where the script's
               re-split of the blank-joined line changes the word count or a token is a run of punctuation
  sets         hypothesis sets (a)-(g) (tests/speaker_bleu_cases.build_results turns one into the results dictionary);
               per instructions_per_path what SpeakerEvaluation.score_results returned: summary, the generated
               instructions (digest), everything it printed
  multi_bleu   hand-made cases with the pair multi_bleu returned
"""
import contextlib
import gzip
import io
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
REF = os.environ.get('SF_REFERENCE', '/root/reference')
SPLIT = 'sub_val_seen'

import speaker_bleu_cases as cases                       # noqa: E402


def hypothesis_sets(items, split_sentence, vocab):
    rng = np.random.default_rng(16)
    known = set(vocab)
    n = len(items)
    scores = lambda: {str(it['path_id']): float(rng.normal(-20.0, 6.0)) for it in items}      # noqa: E731
    sets = []
    # (a) the neighbouring path's first instruction as a speaker over train_vocab.txt would say it
    a = {str(it['path_id']): [w if w in known else '<UNK>' for w in split_sentence(items[(i + 1) % n]['instructions'][0])][:80]
         for i, it in enumerate(items)}
    sets.append(dict(name='a_neighbour', hyps=a, scores=scores(), order='file'))
    # (b) the path's own third instruction cut to 12 words: high precision, the brevity penalty at work
    b = {str(it['path_id']): split_sentence(it['instructions'][2])[:12] for it in items}
    sets.append(dict(name='b_own_third_cut', hyps=b, scores=scores(), order='file'))
    # (c) a mix: empty, 1 / 2 / 3 words (orders without n-grams), one word 40 times (clipping), <UNK> / <EOS> strings
    c = {}
    for i, it in enumerate(items):
        own = split_sentence(it['instructions'][0])
        kind = i % 8
        c[str(it['path_id'])] = ([], own[:1], own[:2], own[:3], ['the'] * 40, ['<UNK>', 'walk', '<EOS>', 'the', '<UNK>'],
                                 own[:30], a[str(it['path_id'])][:25])[kind]
    sets.append(dict(name='c_mix', hyps=c, scores=scores(), order='file'))
    sets.append(dict(name='d_the', hyps={str(it['path_id']): ['the'] for it in items}, scores=scores(), order='file'))
    sets.append(dict(name='e_empty', hyps={str(it['path_id']): [] for it in items}, scores=scores(), order='file'))
    # (f) reversed iteration order, and for some paths one instruction id with other words: where it is the id met
    # first ('_2': the last of the file order, the first of the reversed one) its words are the path's hypothesis,
    # where it is met later ('_1', '_0') it is a reported mismatch
    over = []
    for i, it in enumerate(items[:40]):
        j = (2, 1, 0)[i % 3]
        over.append(['%d_%d' % (it['path_id'], j), split_sentence(it['instructions'][1])[:20], float(-i)])
    sets.append(dict(name='f_duplicates_reversed', hyps=a, scores=sets[0]['scores'], order='reversed', overrides=over))
    sets.append(dict(name='g_no_scores', hyps=b, scores=None, order='file'))
    return sets


def multi_bleu_cases():
    w = 'a b c d e f g h i j k l m n o p'.split()
    return [
        dict(name='tie_8_12', refs=[[w[:8], w[:12]]], hyps=[w[:10]]),
        dict(name='tie_12_8', refs=[[w[:12], w[:8]]], hyps=[w[:10]]),
        dict(name='r1', refs=[[w[:9]], [w[2:8]]], hyps=[w[:7], w[3:8]]),
        dict(name='r2', refs=[[w[:9], w[1:6]], [w[2:8], w[:4]]], hyps=[w[:7], w[3:8]]),
        dict(name='r3', refs=[[w[:9], w[1:6], w[4:16]]], hyps=[w[2:11]]),
        dict(name='r4', refs=[[w[:9], w[1:6], w[4:16], w[:5] + w[7:12]]], hyps=[w[:12]]),
        dict(name='empty_reference', refs=[[[], w[:6]]], hyps=[w[:5]]),
        dict(name='only_empty_references', refs=[[[]], [[]]], hyps=[w[:5], w[:2]]),
        dict(name='hypothesis_longer', refs=[[w[:5], w[:6]]], hyps=[w[:14]]),
        dict(name='clipping_split_maximum', refs=[[list('aaabcd'), list('bbacdb')]],
             hyps=['a a a a b b b c d'.split()]),
        dict(name='clipping_across_references', refs=[['x y x y x y'.split(), 'p q p q x y'.split()]],
             hyps=['x y x y p q p q p q'.split()]),
        dict(name='token_with_a_blank', refs=[[['go', '. .', 'stop'], ['go', '.', '.', 'now']]], hyps=[['go', '.', '.', 'stop']]),
        dict(name='no_match', refs=[[w[:6]]], hyps=[w[8:14]]),
        dict(name='exact', refs=[[w[:10]], [w[3:9]]], hyps=[w[:10], w[3:9]]),
        dict(name='short_hypotheses', refs=[[w[:10]], [w[3:9]], [w[:4]]], hyps=[w[:3], w[3:4], []]),
    ]


def as_json(x):
    x = float(x)
    return None if math.isnan(x) else x


def main():
    sys.path.insert(0, os.path.join(REF, 'tasks', 'R2R'))
    os.chdir(REF)                                          # (load_datasets and the script's path are relative to it)
    import utils as ref_utils
    import eval_speaker as ref_eval
    import bleu as ref_bleu
    raw = ref_utils.load_datasets([SPLIT])
    items = [dict(path_id=it['path_id'], scan=it['scan'], instructions=list(it['instructions'])) for it in raw]
    vocab = ref_utils.read_vocab(os.path.join('tasks', 'R2R', 'data', 'train_vocab.txt'))
    split = ref_utils.Tokenizer.split_sentence

    tokens = {}
    for it in items:
        for j, text in enumerate(it['instructions']):
            toks = split(text)
            rec = dict(digest=cases.digest(toks))
            punct_run = any(len(t) > 1 and not any(c.isalnum() or c == '_' for c in t) for t in toks)
            if len(' '.join(toks).split()) != len(toks) or punct_run:
                rec['tokens'] = toks
            tokens['%d_%d' % (it['path_id'], j)] = rec

    sets = hypothesis_sets(items, split, vocab)
    for case in sets:
        case['want'] = {}
        for ipp in (3, 2, 1) + ((4,) if case['name'] in ('a_neighbour', 'b_own_third_cut') else ()):
            ev = ref_eval.SpeakerEvaluation([SPLIT], instructions_per_path=ipp)
            results = cases.build_results(items, case)
            printed = io.StringIO()
            with contextlib.redirect_stdout(printed), np.errstate(all='ignore'):
                summary, replaced = ev.score_results(results)
            assert [r['path_id'] for r in replaced] == sorted(it['path_id'] for it in items)
            case['want'][str(ipp)] = dict(
                summary={k: as_json(v) for k, v in summary.items()},
                replaced=cases.digest([r['instructions'][0] for r in replaced]),
                printed=printed.getvalue())
            print('%-24s ipp %d: %s  (%d characters printed)' % (case['name'], ipp, summary, len(printed.getvalue())))

    hand = multi_bleu_cases()
    for c in hand:
        c['want'] = [float(x) for x in ref_bleu.multi_bleu(c['refs'], c['hyps'])]
        print('%-28s %s' % (c['name'], c['want']))

    out = dict(source='tasks/R2R/data/R2R_%s.json, train_vocab.txt; outputs of eval_speaker.SpeakerEvaluation.score_results '
                      'and bleu.multi_bleu' % SPLIT,
               items=items, vocab=vocab, tokens=tokens, sets=sets, multi_bleu=hand)
    with gzip.open(cases.PATH, 'wt') as f:
        json.dump(out, f)
    print('wrote', cases.PATH, os.path.getsize(cases.PATH), 'bytes; instructions with tokens in full: %d'
          % sum('tokens' in r for r in tokens.values()))


if __name__ == '__main__':
    main()
