"""CPU: the caption metrics of speaker_follower_amd.speaker_evaluation -- ROUGE-L and CIDEr-D over the BLEU words,
`SpeakerEvaluation(..., caption_metrics=True)` -- against the plain restatement of DESIGN.md section 2 in
tests/caption_metric_cases.py and against answers that can be checked by hand.  The texts are the g16 fixture's
(tests/golden/g16_speaker_bleu.json.gz).  device='cpu' throughout: the host producer caption_parts_rows, which is the
kernel's specification, and caption_scores_of, the one function both paths end in.  Per-path comparisons are `==`: the
package and the restatement form the same products and add them in the order of first occurrence."""
import contextlib
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import caption_metric_cases as cm                                   # noqa: E402
import speaker_bleu_cases as cases                                  # noqa: E402

from speaker_follower_amd import speaker_evaluation as se           # noqa: E402

FX = cases.load()
BLEU_KEYS = ['model_score', 'bleu', 'unpenalized_bleu']


def scores(refs, hyps):
    """(rouge_l, cider_d) per path through the package: parts, static rows, caption_scores_of; corpus = refs."""
    corpus = se.caption_corpus(refs)
    return [se.caption_scores_of(parts, static) for parts, static in
            zip(se.caption_parts_rows(refs, hyps, corpus), se.caption_static_rows(refs, corpus))]


def evaluate(case, ipp, **kw):
    ev = se.SpeakerEvaluation(items=FX['items'], splits=['sub_val_seen'], instructions_per_path=ipp, **kw)
    results = cases.build_results(FX['items'], case)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        summary, replaced = ev.score_results(results)
    return ev, summary, results


def test_known_answers():
    w = 'a b c d e x'.split()
    a, b, c, d, e, x = w
    # a hypothesis equal to one of its references: ROUGE-L exactly 1.0
    refs = [[[a, b, c], [d, e, x, a]], [[x, x], [e]]]
    got = scores(refs, [[d, e, x, a], [a]])
    assert got[0][0] == 1.0 and got[1][0] == 0.0
    # `a b c d` against `a x c d e`: LCS 3, p = 3/4, r = 3/5
    parts = se.caption_parts_rows([[[a, x, c, d, e]]], [[a, b, c, d]])[0]
    assert parts['hyp_len'] == 4 and parts['lcs'] == [3]
    rouge = scores([[[a, x, c, d, e]]], [[a, b, c, d]])[0][0]
    assert abs(rouge - 2.44 * 0.45 / 1.68) < 1e-15 and rouge == cm.rouge_l([a, b, c, d], [[a, x, c, d, e]])
    # two paths, each hypothesis its own single reference: orders 1 and 2 give 1.0, orders 3 and 4 have zero norms
    refs = [[[a, b]], [[c, d]]]
    got = scores(refs, [[a, b], [c, d]])
    for rouge, cider in got:
        assert rouge == 1.0 and abs(cider - 5.0) < 1e-14
    parts = se.caption_parts_rows(refs, [[a, b], [c, d]])
    assert parts[0]['hnorm2'][2:] == [0.0, 0.0] and parts[0]['dot'][0][2:] == [0.0, 0.0]
    log2 = math.log(2)
    assert parts[0]['hnorm2'][0] == log2 * log2 + log2 * log2 and parts[0]['hnorm2'][1] == log2 * log2
    # a corpus of one path: every idf is log 1 - log 1
    assert scores([[[a, b, c]]], [[a, b, c]])[0] == (1.0, 0.0)
    # the empty hypothesis: 0.0 for both
    assert scores(refs, [[], [c]])[0] == (0.0, 0.0)
    assert se.caption_parts_rows(refs, [[], [c]])[0] == dict(hyp_len=0, lcs=[0], dot=[[0.0] * 4], hnorm2=[0.0] * 4)
    # an n-gram no reference holds has df 0: idf log N; clipping on both sides of tf_r
    refs = [[[a, a, b]], [[c]], [[d]]]
    parts = se.caption_parts_rows(refs, [[a, a, a, x], [c], [d]])[0]
    log3 = math.log(3)
    assert parts['hnorm2'][0] == (3 * log3) * (3 * log3) + log3 * log3  # 'a' three times, 'x' unseen
    assert parts['dot'][0][0] == (2 * log3) * (2 * log3)                # tf_h 3 above tf_r 2: clipped to the reference's
    parts = se.caption_parts_rows(refs, [[a, b], [c], [d]])[0]
    assert parts['dot'][0][0] == (1 * log3) * (2 * log3) + log3 * log3  # tf_h 1 below tf_r 2


@pytest.mark.parametrize('ipp', [1, 2, 3])
@pytest.mark.parametrize('name', [c['name'] for c in FX['sets']])
def test_score_results_equals_the_restatement(name, ipp):
    case = next(c for c in FX['sets'] if c['name'] == name)
    ev, summary, results = evaluate(case, ipp, device='cpu', caption_metrics=True)
    assert list(summary) == BLEU_KEYS + ['rouge_l', 'cider_d']
    scored = sorted(it['path_id'] for it in FX['items'] if len(it['instructions'][:ipp]) == ipp)
    assert len(scored) == 260 and sorted(ev.counts['rows']) == scored      # the paths BLEU scores
    assert sorted(ev.captions['parts']) == scored and sorted(ev.captions['on_host']) == scored
    first = cm.first_hypotheses(results, ev.instr_ids)
    refs = [[se.bleu_words(se.split_sentence(r)) for r in ev.gt[pid]['instructions']] for pid in scored]
    hyps = [se.bleu_words(first[pid]) for pid in scored]
    assert all(len(r) == ipp for r in refs)
    rouge, cider = cm.score(refs, hyps)
    for i, pid in enumerate(scored):
        assert ev.captions['rouge_l'][pid] == rouge[i], (pid, ev.captions['rouge_l'][pid], rouge[i])
        assert ev.captions['cider_d'][pid] == cider[i], (pid, ev.captions['cider_d'][pid], cider[i])
        assert ev.captions['parts'][pid]['hyp_len'] == len(hyps[i]) == ev.counts['rows'][pid][8]
    assert summary['rouge_l'] == cm.mean(rouge) and summary['cider_d'] == cm.mean(cider)
    assert 0.0 <= min(rouge) and max(rouge) <= 1.0 and 0.0 <= min(cider) and max(cider) < 10.0 + 1e-12  # (a quotient of rounded norms)
    if name == 'e_empty':
        assert summary['rouge_l'] == 0.0 and summary['cider_d'] == 0.0
    if name == 'b_own_third_cut' and ipp == 3:                       # (a cut of the third reference)
        assert summary['rouge_l'] > 0.3 and summary['cider_d'] > 0.3


def test_paths_without_all_references_are_outside_the_corpus():
    case = FX['sets'][0]
    ev, summary, _ = evaluate(case, 4, device='cpu', caption_metrics=True)
    scored = sorted(it['path_id'] for it in FX['items'] if len(it['instructions']) >= 4)
    assert len(scored) == 2 and sorted(ev.captions['parts']) == scored == sorted(ev.counts['rows'])
    assert ev._caption['corpus']['n_paths'] == 2 and ev._caption['corpus']['log_n'] == math.log(2)


def test_the_switch_is_off_by_default_and_changes_nothing():
    case = FX['sets'][2]
    plain, want, _ = evaluate(case, 3, device='cpu')
    off, got, _ = evaluate(case, 3, device='cpu', caption_metrics=False)
    on, with_captions, _ = evaluate(case, 3, device='cpu', caption_metrics=True)
    assert list(want) == list(got) == BLEU_KEYS and plain.captions is None and off.captions is None
    for k in BLEU_KEYS:
        assert got[k] == want[k] == with_captions[k]
    for ev in (off, on):
        assert sorted(ev.counts) == sorted(plain.counts) and ev.counts['on_host'] == plain.counts['on_host']
        assert ev.counts['sums'].tolist() == plain.counts['sums'].tolist()
        assert list(ev.counts['rows']) == list(plain.counts['rows'])
        assert all(ev.counts['rows'][p].tolist() == r.tolist() for p, r in plain.counts['rows'].items())
    assert plain._caption is None and off._caption is None              # nothing was even built


@pytest.mark.parametrize('limits', [(65536, 25, 40, 4), (300, 256, 512, 4), (65536, 256, 512, 2), (65536, 256, 512, 4)])
def test_paths_above_the_limits_are_formed_on_the_host_and_merged(monkeypatch, limits):
    """_caption_parts' partition, dictionary and key tables, with caption_parts_rows over the ids standing in for the
    kernel: what goes to the device is ids inside the limits and tables that decode to the corpus' idf; the rest is
    formed on the host; the merge equals the all-host evaluator, `==`."""
    sent = []

    def rows_stand_in(ref_ids, hyp_ids, R, n_dict, dev):
        return se.bleu_count_rows([ref_ids[i * R:(i + 1) * R] for i in range(len(hyp_ids))], hyp_ids)

    def parts_stand_in(ref_ids, hyp_ids, R, n_dict, tables, dev):
        sent.append((len(hyp_ids), n_dict))
        assert R <= limits[3] and n_dict <= limits[0] and max(len(h) for h in hyp_ids) <= limits[1]
        assert max(len(r) for r in ref_ids) <= limits[2] and max(max(s) for s in ref_ids + hyp_ids if s) < n_dict
        keys, idf, first = tables['keys'].tolist(), tables['idf'].tolist(), 0
        corpus = dict(log_n=tables['log_n'], idf=[])
        for n, count in enumerate(tables['n_keys'], 1):
            mine = keys[first:first + count]
            assert mine == sorted(set(mine)) and all(k >> (16 * n) == 0 for k in mine)
            corpus['idf'].append({tuple((k >> (16 * j)) & 0xffff for j in range(n)): v
                                  for k, v in zip(mine, idf[first:first + count])})
            first += count
        return se.caption_parts_rows([ref_ids[i * R:(i + 1) * R] for i in range(len(hyp_ids))], hyp_ids, corpus)
    case = FX['sets'][0]
    host, want, _ = evaluate(case, 3, device='cpu', caption_metrics=True)
    monkeypatch.setattr(se, '_cuda_device', lambda device: 'stand-in')
    monkeypatch.setattr(se, '_device_rows', rows_stand_in)
    monkeypatch.setattr(se, '_device_parts', parts_stand_in)
    monkeypatch.setattr(se, 'bleu_limits', lambda: limits)
    ev, got, _ = evaluate(case, 3, device=None, caption_metrics=True)
    assert got == want
    assert ev.captions['parts'] == host.captions['parts'] and ev.captions['cider_d'] == host.captions['cider_d']
    assert ev.captions['rouge_l'] == host.captions['rouge_l']
    n_host = len(ev.captions['on_host'])
    n_ref_words = len(ev._caption['ids'])
    assert n_ref_words > 300
    if limits == (65536, 256, 512, 4):
        assert n_host == 0 and sent == [(260, sent[0][1])] and sent[0][1] >= n_ref_words
    elif limits[3] == 2 or limits[0] == 300:                           # no room for three references / for the tables
        assert n_host == 260 and sent == []
    else:
        assert 0 < n_host < 260 and sent[0][0] == 260 - n_host
        assert ev.captions['on_host'] == sorted(ev.captions['on_host'])


def test_compat_module_exports_the_new_names():
    compat = os.path.join(cases.ROOT, 'speaker_follower_amd', 'compat')
    code = ('import sys; sys.path.insert(0, %r); import eval_speaker as es; '
            'assert "torch" not in sys.modules; '
            'refs = [[["a", "b"]], [["c", "d"]]]; corpus = es.caption_corpus(refs); '
            'parts = es.caption_parts_rows(refs, [["a", "b"], ["c", "d"]], corpus); '
            'static = es.caption_static_rows(refs, corpus); '
            'print(es.caption_scores_of(parts[0], static[0])[0], '
            'es.SpeakerEvaluation(items=[], caption_metrics=True).caption_metrics)' % compat)
    out = subprocess.run([sys.executable, '-c', code], cwd=cases.ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == '1.0 True'
