"""CPU: speaker_follower_amd.speaker_evaluation against what the reference's eval_speaker.SpeakerEvaluation and
bleu.multi_bleu returned (tests/golden/g16_speaker_bleu.json.gz, written by tests/golden/make_golden_bleu.py on the
split the reference ships).  Corpus BLEU is a function of ten integers, so every comparison is `==`: the three numbers
of a summary, the generated instructions, everything score_results prints.  Nothing here reads the reference, runs
perl or touches a GPU (device='cpu': the host counting, which is the kernel's specification)."""
import contextlib
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import speaker_bleu_cases as cases                                  # noqa: E402

from speaker_follower_amd import speaker_evaluation as se           # noqa: E402

FX = cases.load()
SETS = [(c['name'], ipp) for c in FX['sets'] for ipp in sorted(c['want'])]


def same_number(got, want):
    """== on doubles; the reference's nan (np.mean of no scores) is recorded as null."""
    if want is None:
        return isinstance(got, float) and math.isnan(got)
    return got == want


def score(case, ipp, device='cpu'):
    ev = se.SpeakerEvaluation(items=FX['items'], splits=['sub_val_seen'], instructions_per_path=ipp, device=device)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed), np.errstate(all='ignore'):
        summary, replaced = ev.score_results(cases.build_results(FX['items'], case))
    return ev, summary, replaced, printed.getvalue()


def check_against_golden(case, ipp, device='cpu'):
    want = case['want'][ipp]
    ev, summary, replaced, printed = score(case, int(ipp), device)
    assert set(summary) == {'model_score', 'bleu', 'unpenalized_bleu'}
    for k, v in want['summary'].items():
        assert same_number(float(summary[k]), v), (k, summary[k], v)
    assert [r['path_id'] for r in replaced] == sorted(it['path_id'] for it in FX['items'])
    assert cases.digest([r['instructions'][0] for r in replaced]) == want['replaced']
    assert all(set(r) == set(ev.gt[r['path_id']]) for r in replaced)
    assert printed == want['printed']
    return ev, summary


def test_module_imports_without_torch_and_without_the_reference():
    code = ('import sys; import speaker_follower_amd.speaker_evaluation as se; '
            'assert "torch" not in sys.modules and "utils" not in sys.modules and "bleu" not in sys.modules; '
            'print(se.multi_bleu([[["a", "b", "c", "d", "e"]]], [["a", "b", "c", "d", "e"]]))')
    out = subprocess.run([sys.executable, '-c', code], cwd=cases.ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == '(100.0, 100.0)'


def test_tokeniser_pins():
    full = 0
    for it in FX['items']:
        for j, text in enumerate(it['instructions']):
            rec = FX['tokens']['%d_%d' % (it['path_id'], j)]
            toks = se.split_sentence(text)
            assert cases.digest(toks) == rec['digest'], (it['path_id'], j)
            if 'tokens' in rec:
                full += 1
                assert toks == rec['tokens']
    assert full >= 1
    assert se.split_sentence('  Walk!? past.. the  "sofa", stop ') == ['walk', '!', '?', 'past', '..', 'the', '"', 'sofa',
                                                                       '"', ',', 'stop']
    # the script splits the blank-joined line again: a token that holds a blank is two words, an empty one none
    blank = [t for rec in FX['tokens'].values() for t in rec.get('tokens', []) if ' ' in t]
    assert len(blank) == 1
    assert se.bleu_words(['go', blank[0], 'stop', '']) == ['go'] + blank[0].split(' ') + ['stop']
    assert se.bleu_words(['a\tb', 'c d']) == ['a', 'b', 'c d']      # (bytes: only ASCII white space splits)


@pytest.mark.parametrize('name,ipp', SETS)
def test_score_results_equals_the_reference(name, ipp):
    case = next(c for c in FX['sets'] if c['name'] == name)
    ev, summary = check_against_golden(case, ipp)
    scored = [it['path_id'] for it in FX['items'] if len(it['instructions'][:int(ipp)]) == int(ipp)]
    assert sorted(ev.counts['rows']) == sorted(scored) and sorted(ev.counts['on_host']) == sorted(scored)
    assert ev.skipped == sorted(set(it['path_id'] for it in FX['items']) - set(scored))
    assert (ev.counts['sums'] == np.sum([ev.counts['rows'][p] for p in scored], axis=0, dtype=np.int64)).all()
    assert se.bleu_from_counts(ev.counts['sums'])[:2] == (summary['bleu'], summary['unpenalized_bleu'])


@pytest.mark.parametrize('limits', [(65536, 25, 40, 4), (300, 256, 512, 4), (65536, 256, 512, 2), (65536, 256, 512, 4)])
def test_paths_above_the_limits_are_counted_on_the_host_and_merged(monkeypatch, limits):
    """count_rows' partition and its dictionary, with bleu_count_rows over the ids standing in for the kernel: what
    goes to the device is ids by string, inside the limits; the rest is counted on the host; the merge is golden."""
    sent = []

    def stand_in(ref_ids, hyp_ids, R, n_dict, dev):
        sent.append((len(hyp_ids), n_dict))
        assert R <= limits[3] and n_dict <= limits[0] and max(len(h) for h in hyp_ids) <= limits[1]
        assert max(len(r) for r in ref_ids) <= limits[2] and max(max(s) for s in ref_ids + hyp_ids if s) < n_dict
        return se.bleu_count_rows([ref_ids[i * R:(i + 1) * R] for i in range(len(hyp_ids))], hyp_ids)
    monkeypatch.setattr(se, '_cuda_device', lambda device: 'stand-in')
    monkeypatch.setattr(se, '_device_rows', stand_in)
    monkeypatch.setattr(se, 'bleu_limits', lambda: limits)
    ev, _ = check_against_golden(FX['sets'][0], '3', device=None)
    n_host = len(ev.counts['on_host'])
    if limits == (65536, 256, 512, 4):
        assert n_host == 0 and sent == [(260, sent[0][1])]
    elif limits[3] == 2:
        assert n_host == 260 and sent == []
    else:
        assert 0 < n_host < 260 and sent[0][0] == 260 - n_host


def test_the_cases_cover_what_they_are_there_for():
    want = {c['name']: c['want'] for c in FX['sets']}
    assert want['a_neighbour']['3']['summary']['bleu'] == 7.99 == want['a_neighbour']['3']['summary']['unpenalized_bleu']
    b = want['b_own_third_cut']['3']['summary']
    assert b['bleu'] < 0.5 * b['unpenalized_bleu']                   # the brevity penalty at work
    assert want['d_the']['3']['summary']['bleu'] == 0 and want['e_empty']['3']['summary']['bleu'] == 0
    assert 'mismatching outputs' in want['f_duplicates_reversed']['3']['printed']
    assert want['f_duplicates_reversed']['1']['printed'] == ''
    assert want['f_duplicates_reversed']['3']['summary'] != want['a_neighbour']['3']['summary']   # the first id met wins
    assert want['g_no_scores']['3']['summary']['model_score'] is None
    assert want['a_neighbour']['4']['printed'].startswith('skipped 258 instructions without 4 refs:')
    ev, _, _, _ = score(next(c for c in FX['sets'] if c['name'] == 'c_mix'), 3)
    rows = np.array(list(ev.counts['rows'].values()))
    assert (rows[:, 8] == 0).any() and ((rows[:, 8] == 1) & (rows[:, 5] == 0)).any() and (rows[:, 8] == 40).any()
    assert (rows[rows[:, 8] == 40][:, 0] < 40).all()                 # 'the' x 40: clipped at the references' count


@pytest.mark.parametrize('case', FX['multi_bleu'], ids=[c['name'] for c in FX['multi_bleu']])
def test_multi_bleu_equals_the_reference(case):
    got = se.multi_bleu(case['refs'], case['hyps'])
    assert [float(x) for x in got] == case['want']
    if len(case['refs'][0]) == 1:
        assert se.single_bleu([r[0] for r in case['refs']], case['hyps']) == got


def test_closest_length_tie_takes_the_shorter_reference():
    w = list('abcdefghijkl')
    for refs in ([w[:8], w[:12]], [w[:12], w[:8]]):
        assert se.bleu_count_rows([refs], [w[:10]])[0, 9] == 8
    assert se.bleu_count_rows([[w[:12], w[:11]]], [w[:10]])[0, 9] == 11
    # different references hold the maximum for different n-grams
    rows = se.bleu_count_rows([[list('aaabcd'), list('bbacdb')]], [list('aaaabbbcd')])
    assert rows[0].tolist() == [3 + 3 + 1 + 1, 2 + 1 + 1 + 1 + 1, 1 + 1 + 1, 1, 9, 8, 7, 6, 9, 6]


def test_missing_ids_raise_the_references_message():
    case = FX['sets'][0]
    ev = se.SpeakerEvaluation(items=FX['items'], splits=['sub_val_seen'], device='cpu')
    results = cases.build_results(FX['items'], case)
    gone = [k for k in list(results) if k in ev.instr_ids][:5]
    for k in gone:
        del results[k]
    with pytest.raises(AssertionError) as e:
        ev.score_results(results)
    assert str(e.value) == 'Missing 5 of %d instruction ids from sub_val_seen' % len(ev.instr_ids)
    assert len(ev.instr_ids) == 3 * 260 and ev.instructions_per_path == 3 and len(ev.scans) == 51 and len(ev.gt) == 260


def test_bleu_from_counts_edges():
    # no reference words at all: the script prints "BLEU = 0, ... BP=0"
    bleu, unpenalized, rec = se.bleu_from_counts([0, 0, 0, 0, 5, 4, 3, 2, 5, 0])
    assert (bleu, unpenalized) == (0, 0) and rec['ref_len'] == 0 and rec['hyp_len'] == 5
    # no hypothesis words with reference words: the script dies on 1 - ref_len / 0, call_bleu returns (0, 0)
    bleu, unpenalized, rec = se.bleu_from_counts([0] * 9 + [7])
    assert (bleu, unpenalized) == (0, 0) and rec['bleu_exact'] == 0.0 and rec['precisions'] == [0.0] * 4
    # an order without a match: exp(-9999999999 / 4) is 0
    assert se.bleu_from_counts([3, 2, 1, 0, 4, 3, 2, 1, 4, 4])[:2] == (0.0, 0.0)
    # the pair is made of the ROUNDED numbers; the record keeps the exact ones
    bleu, unpenalized, rec = se.bleu_from_counts([10, 9, 8, 7, 10, 9, 8, 7, 10, 12])
    bp = math.exp(1 - 12 / 10)
    assert rec['brevity_penalty'] == bp and rec['bleu_exact'] == bp * math.exp(0.0) and rec['precisions'] == [1.0] * 4
    assert bleu == float('%.2f' % (100 * bp)) == 81.87 and unpenalized == 81.87 / float('%.3f' % bp)
    assert se.bleu_from_counts(np.array([10, 9, 8, 7, 10, 9, 8, 7, 10, 10], np.int64))[:2] == (100.0, 100.0)


def test_constructor_forms():
    class Env:
        splits = ['sub_val_seen']
        data = [dict(path_id=it['path_id'], scan=it['scan'], instr_id='%d_%d' % (it['path_id'], j), instructions=text)
                for it in FX['items'] for j, text in enumerate(it['instructions'])]
    Env.data = Env.data[::-1]                                       # (an env shuffles its items)
    by_env = se.SpeakerEvaluation(env=Env(), device='cpu')
    by_items = se.SpeakerEvaluation(items=FX['items'], device='cpu')
    assert by_env.instr_ids == by_items.instr_ids and by_env.scans == by_items.scans and by_env.splits == ['sub_val_seen']
    for pid, gt in by_items.gt.items():
        assert by_env.gt[pid]['instructions'] == gt['instructions'] and len(gt['instructions']) == 3
    two = se.SpeakerEvaluation(items=FX['items'], instructions_per_path=2, device='cpu')
    assert len(two.instr_ids) == 2 * 260 and FX['items'][0]['instructions'] != two.gt[FX['items'][0]['path_id']]['instructions']


def test_compat_imports_resolve_to_the_package(tmp_path):
    data = tmp_path / 'tasks' / 'R2R' / 'data'
    data.mkdir(parents=True)
    (data / 'R2R_sub_val_seen.json').write_text(json.dumps(FX['items']))
    case = FX['sets'][0]
    (tmp_path / 'results.json').write_text(json.dumps(cases.build_results(FX['items'], case)))
    compat = os.path.join(cases.ROOT, 'speaker_follower_amd', 'compat')
    code = ('import sys, json; sys.path.insert(0, %r); sys.path.insert(1, %r); import eval_speaker, bleu; '
            'from bleu import multi_bleu, single_bleu; '
            'import speaker_follower_amd.speaker_evaluation as se; '
            'assert eval_speaker.SpeakerEvaluation is se.SpeakerEvaluation and multi_bleu is se.multi_bleu '
            'and bleu.single_bleu is se.single_bleu; '
            'ev = eval_speaker.SpeakerEvaluation(["sub_val_seen"]); '
            'summary, _ = ev.score_file("results.json"); '
            'print(json.dumps({k: float(v) for k, v in summary.items()}))' % (compat, cases.ROOT))
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
    out = subprocess.run([sys.executable, '-c', code], cwd=str(tmp_path), capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1]) == case['want']['3']['summary']
