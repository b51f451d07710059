"""GPU: sf_caption_scores (csrc/sf_caption.hip) alone against speaker_evaluation.caption_parts_rows (the kernel's
specification), `SpeakerEvaluation(caption_metrics=True).score_results` forming the parts on the device, and
`score_speaker` with the switch on, end to end.

What is compared, and how tightly: hyp_len and lcs with `==`; rouge_l with `==` (a function of integers through the
one host function caption_scores_of); dot, hnorm2, per-path cider_d and the corpus means within 1e-11 absolute of
the host values.  That bound is derived, not measured: each sum has at most 256 non-negative float64 terms, so its
relative error is below 258 * 2^-53 ~ 3e-14 whatever the order; the quotient, the products and the means add a few
ulp; a path's score is at most 10: under 1e-12, and the tests allow ten times that.  dot and hnorm2 are held to the
same absolute bound.  They are no scores but sums of (tf idf)^2, which grow with the sentence, so the kernel cases at
the long lengths take their tables from a corpus whose idf values are scaled down (`scaled`: the kernel is handed
tables, whatever they hold) and `check` asserts that every sum stays below 300, where 258 * 2^-53 * 300 < 1e-11.

Behind every output array stand sentinels, NaN and a large value in turn; slots nobody owns keep theirs."""
import ctypes as C
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import speaker_bleu_cases as cases                                  # noqa: E402
import test_gpu_speaker_evaluation as world                         # noqa: E402  (the 8-scan speaker world)

from speaker_follower_amd import speaker_evaluation as se           # noqa: E402

DEV = torch.device('cuda', 0)
FX = cases.load()
BIG = 65535
TOL = 1e-11
INT_SENTINEL, BIG_SENTINEL = -7, 1e300
GUARD = 8                                                           # sentinels behind every output array
BLEU_KEYS = ['model_score', 'bleu', 'unpenalized_bleu']


class Identity:
    """word -> id for sentences that are ids already."""

    def __getitem__(self, w):
        return int(w)


def launch(refs, hyps=None, corpus=None, slots=None, n_slots=None, n_dict=BIG + 1, words=None, eos=2, remap=None,
           max_hyp=None, max_ref=None):
    """sf_caption_scores once.  refs: per slot R id lists; hyps: id lists (packed form) or `words` [S, B] (matrix
    form) with `remap`; corpus: a caption_corpus over id sentences.  Returns (status, out, err): out holds the four
    arrays over their sentinels, guards included."""
    from speaker_follower_amd import _lib
    R = len(refs[0])
    n_slots = len(refs) if n_slots is None else n_slots
    B = len(hyps) if words is None else words.shape[1]
    slots = np.arange(B, dtype=np.int32) if slots is None else np.asarray(slots, np.int32)
    tables = se.caption_key_tables(corpus, Identity())
    r_ids, r_off = se._packed([r for rs in refs for r in rs])
    h_ids, h_off = se._packed(hyps if words is None else [[]] * B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                      # noqa: E731
    d = dict(r_ids=up(r_ids), r_off=up(r_off), h_ids=up(h_ids), h_off=up(h_off), slot=up(slots),
             keys=up(tables['keys'].view(np.int64)), idf=up(tables['idf']))
    sizes = dict(hyp_len=n_slots, lcs=n_slots * R, dot=n_slots * R * 4, hnorm2=n_slots * 4)
    out = {}
    for name, n in sizes.items():
        if name in ('hyp_len', 'lcs'):
            out[name] = torch.full((n + GUARD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
            out[name][n:] = 2 ** 30
        else:
            out[name] = torch.full((n + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
            out[name][1::2] = BIG_SENTINEL
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    k = tables['n_keys']
    b = _lib.CaptionBatch(n_hyps=B, n_slots=n_slots, n_refs=R, n_dict=n_dict,
                          max_hyp=int(np.diff(h_off).max()) if max_hyp is None else max_hyp,
                          max_ref=int(np.diff(r_off).max()) if max_ref is None else max_ref,
                          ref_ids=d['r_ids'].data_ptr(), ref_off=d['r_off'].data_ptr(), slot=d['slot'].data_ptr(),
                          n_keys1=k[0], n_keys2=k[1], n_keys3=k[2], n_keys4=k[3], keys=d['keys'].data_ptr(),
                          idf=d['idf'].data_ptr(), idf_miss=corpus['log_n'], hyp_len=out['hyp_len'].data_ptr(),
                          lcs=out['lcs'].data_ptr(), dot=out['dot'].data_ptr(), hnorm2=out['hnorm2'].data_ptr())
    if words is None:
        b.hyp_ids, b.hyp_off = d['h_ids'].data_ptr(), d['h_off'].data_ptr()
    else:
        d['words'], d['remap'] = up(words), up(np.asarray(remap, np.int32))
        b.words, b.remap, b.S, b.eos, b.n_vocab = d['words'].data_ptr(), d['remap'].data_ptr(), words.shape[0], eos, len(remap)
        b.word_bytes = words.dtype.itemsize
    status = _lib.lib.sf_caption_scores(C.byref(b), C.c_void_p(err.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status, {name: t.cpu().numpy() for name, t in out.items()}, int(err.item())


def untouched(a, rows, width):
    """Do the `width` values of every row in `rows` of output array `a` (and its guard) still hold their sentinels?"""
    a = np.asarray(a)
    n = len(a) - GUARD
    at = np.concatenate([np.arange(r * width, (r + 1) * width) for r in rows] + [np.arange(n, n + GUARD)]).astype(int)
    if a.dtype == np.int32:
        want = np.where(at >= n, 2 ** 30, INT_SENTINEL)
        return bool((a[at] == want).all())
    odd = at % 2 == 1
    return bool((a[at][odd] == BIG_SENTINEL).all() and np.isnan(a[at][~odd]).all())


def nothing_written(out, n_slots, R):
    return all(untouched(out[name], range(n_slots), w) for name, w in
               (('hyp_len', 1), ('lcs', R), ('dot', R * 4), ('hnorm2', 4)))


def compare(got, want, static=None):
    """One path: the device's parts against the host's, and the scores both give through caption_scores_of."""
    assert got['hyp_len'] == want['hyp_len'] and got['lcs'] == want['lcs'], (got, want)
    for a, b in zip(got['hnorm2'] + [x for d in got['dot'] for x in d], want['hnorm2'] + [x for d in want['dot'] for x in d]):
        assert abs(a - b) <= TOL, (a, b, got, want)
    if static is not None:
        (rouge_d, cider_d), (rouge_h, cider_h) = se.caption_scores_of(got, static), se.caption_scores_of(want, static)
        assert rouge_d == rouge_h and abs(cider_d - cider_h) <= TOL, (rouge_d, rouge_h, cider_d, cider_h)


def check(refs, hyps, corpus=None, slots=None, n_slots=None, **kw):
    """The launch against caption_parts_rows: owned slots equal, slots nobody owns and the guards untouched."""
    corpus = se.caption_corpus(refs) if corpus is None else corpus
    status, out, err = launch(refs, hyps, corpus, slots=slots, n_slots=n_slots, **kw)
    assert status == 0 and err == 0
    R = len(refs[0])
    n = len(refs) if n_slots is None else n_slots
    slots = list(range(len(hyps))) if slots is None else list(slots)
    live = [(b, s) for b, s in enumerate(slots) if s >= 0]
    want = se.caption_parts_rows([refs[s] for _, s in live], [hyps[b] for b, _ in live], corpus)
    static = se.caption_static_rows([refs[s] for _, s in live], corpus)
    got = se._parts_of(out['hyp_len'][:n], out['lcs'][:n * R].reshape(n, R), out['dot'][:n * R * 4].reshape(n, R, 4),
                       out['hnorm2'][:n * 4].reshape(n, 4))
    for (b, s), w, st in zip(live, want, static):
        assert max(w['hnorm2']) < 300 and max(x for d in w['dot'] for x in d) < 300, w
        compare(got[s], w, st)
    idle = sorted(set(range(n)) - {s for _, s in live})
    assert nothing_written(out, 0, R)                                # (the guards)
    for name, w in (('hyp_len', 1), ('lcs', R), ('dot', R * 4), ('hnorm2', 4)):
        assert untouched(out[name], idle, w), name
    return want


def scaled(corpus, by):
    """The corpus with every idf (and the idf of an unseen n-gram) multiplied by `by`: zeros stay zeros."""
    return dict(corpus, log_n=corpus['log_n'] * by, idf=[{g: v * by for g, v in t.items()} for t in corpus['idf']])


def sentence(rng, n, alphabet):
    return [int(alphabet[i]) for i in rng.integers(len(alphabet), size=n)]


HYP_LENS = [0, 1, 3, 4, 63, 64, 65, 255, 256]
REF_LENS = [1, 63, 64, 65, 511, 512]
DENSE = [0, 5, 9, BIG]                                              # dense in repeats; the smallest and largest id
WIDE = list(range(1, 40)) + [BIG]


def test_every_length_edge_with_one_reference():
    rng = np.random.default_rng(1)
    refs, hyps = [], []
    for h in HYP_LENS:
        for r in REF_LENS:
            alphabet = DENSE if (len(refs) % 2) else WIDE
            refs.append([sentence(rng, r, alphabet)])
            hyps.append(sentence(rng, h, alphabet))
    # a hypothesis that IS its reference at both limits' edge, and one that shares no word with it
    refs.append([sentence(rng, 256, WIDE)])
    hyps.append(list(refs[-1][0]))
    refs.append([sentence(rng, 30, WIDE[:10])])
    hyps.append(sentence(rng, 30, WIDE[20:30]))
    want = check(refs, hyps, corpus=scaled(se.caption_corpus(refs), 0.1))
    assert want[-2]['lcs'] == [256] and want[-1]['lcs'] == [0] and want[-1]['dot'] == [[0.0] * 4]
    assert [w['hyp_len'] for w in want[:len(HYP_LENS) * len(REF_LENS)]] == [h for h in HYP_LENS for _ in REF_LENS]
    three = want[2 * len(REF_LENS)]
    assert three['hyp_len'] == 3 and three['hnorm2'][3] == 0.0 and three['hnorm2'][2] > 0     # length 3 has no 4-gram
    assert any(w['dot'][0][3] > 0 for w in want) and any(0 < w['lcs'][0] < w['hyp_len'] for w in want)


@pytest.mark.parametrize('R', [2, 3, 4])
def test_length_edges_with_several_references(R):
    rng = np.random.default_rng(10 + R)
    refs, hyps = [], []
    for k in range(2 * len(HYP_LENS)):                              # every hypothesis length twice, the reference
        alphabet = DENSE if k % 2 else WIDE                         # lengths in turn: every one in every position
        refs.append([sentence(rng, REF_LENS[(k + j * (k // 6 + 1)) % 6], alphabet) for j in range(R)])
        hyps.append(sentence(rng, HYP_LENS[k % len(HYP_LENS)], alphabet))
    refs.append([sentence(rng, 40, WIDE) for _ in range(R)])
    hyps.append(list(refs[-1][R - 1]))                              # equal to its LAST reference
    want = check(refs, hyps, corpus=scaled(se.caption_corpus(refs), 0.1))
    assert want[-1]['lcs'][R - 1] == 40 and {len(r) for rs in refs for r in rs} >= set(REF_LENS)
    assert any(len(set(w['lcs'])) > 1 for w in want)


def test_repeats_clipping_and_order_confusion():
    x = 77
    refs = [[[7, 7, 7, 1, 2], [7, 3]],                              # 0: hypothesis 7 x 8: tf_h above tf_r in both
            [[8, 8, 8, 8, 8], [8, 4]],                              # 1: hypothesis 8 8: tf_h below tf_r 5, above tf_r 1
            [[x, 0, 0, 0, 9], [9, 9]],                              # 2: the 2-gram (x, 0) beside the 4-gram (x, 0, 0, 0)
            [[x, 0, 6], [6, x, 0]],                                 # 3: ... whose 2-gram is in two paths
            [[11, 12, 13, 14, 11, 12, 13, 14], [11, 12]],           # 4: a repeated 4-gram
            [[20, 21], [22]]]
    hyps = [[7] * 8, [8, 8], [x, 0], [x, 0, 0, 0], [11, 12, 13, 14] * 3, [0, BIG, 0]]
    corpus = se.caption_corpus(refs)
    assert corpus['idf'][1][(x, 0)] != corpus['idf'][3][(x, 0, 0, 0)]           # the keys pack alike, the idf differ
    want = check(refs, hyps)
    assert want[0]['dot'][0][0] > want[0]['dot'][1][0] > 0 and want[0]['hnorm2'][3] > 0
    assert want[1]['dot'][0][0] > 0 and want[1]['dot'][1][0] > 0 and want[1]['dot'][0][0] != want[1]['dot'][1][0]
    assert want[2]['hnorm2'][1] > 0 and want[2]['hnorm2'][3] == 0 and want[3]['hnorm2'][3] > 0
    assert want[4]['dot'][0][3] > 0 and want[5]['lcs'] == [0, 0]


def test_table_look_ups():
    rng = np.random.default_rng(5)
    # the corpus is larger than the paths launched: n-grams in a table but in none of this path's references
    others = [[sentence(rng, 12, WIDE[:12]), sentence(rng, 9, WIDE[:12])] for _ in range(20)]
    refs = [[[0], [BIG, BIG, BIG, BIG]],                            # the first key of table 1, the last of table 4
            [sentence(rng, 10, WIDE[:6]), sentence(rng, 10, WIDE[:6])],
            [[30, 31, 32], [33]]]
    hyps = [[0, BIG, BIG, BIG, BIG],
            sentence(rng, 20, WIDE[:12]),                           # words of the others' references
            [900, 901, 902, 903, 904]]                              # n-grams absent from every table
    corpus = se.caption_corpus(refs + others)
    tables = se.caption_key_tables(corpus, Identity())
    assert tables['keys'][0] == 0 and int(tables['keys'][-1]) == 2 ** 64 - 1
    want = check(refs, hyps, corpus=corpus)
    log_n = math.log(23)
    assert want[0]['dot'][0][0] > 0 and want[0]['dot'][1][3] > 0
    assert any((w,) in corpus['idf'][0] and not any(w in r for r in refs[1]) for w in hyps[1]) and max(want[1]['lcs']) > 0
    assert abs(want[2]['hnorm2'][0] - 5 * log_n ** 2) < 1e-12 and want[2]['dot'] == [[0.0] * 4] * 2
    # a table of one key (orders 2..4 hold none), hit and missed
    one = dict(n_paths=4, log_n=math.log(4), idf=[{(5,): 0.625}, {}, {}, {}])
    want = check([[[5, 5, 6]], [[6]]], [[5, 6, 5], [4, 6]], corpus=one)
    assert want[0]['dot'][0][0] == (2 * 0.625) * (2 * 0.625) + one['log_n'] * one['log_n'] and want[0]['hnorm2'][1] > 0


@pytest.mark.parametrize('n_paths', [1, 63, 64, 65, 257])
def test_path_counts_and_interleaved_empty_slots(n_paths):
    rng = np.random.default_rng(100 + n_paths)
    alphabet = list(range(12))
    refs = [[sentence(rng, int(rng.integers(1, 40)), alphabet) for _ in range(3)] for _ in range(n_paths)]
    B = n_paths + n_paths // 2 + 1                                  # more hypotheses than paths: the others hold -1
    slots = np.full(B, -1, np.int64)
    slots[rng.permutation(B)[:n_paths]] = rng.permutation(n_paths)
    hyps = [sentence(rng, int(rng.integers(0, 45)), alphabet) for _ in range(B)]
    corpus = scaled(se.caption_corpus(refs), 0.25)
    check(refs, hyps, corpus=corpus, slots=slots.tolist(), n_slots=n_paths)
    # two slots behind the paths that nobody owns
    check(refs + [[[1], [2], [3]]] * 2, hyps[:n_paths], corpus=corpus, slots=list(range(n_paths)), n_slots=n_paths + 2)


@pytest.mark.parametrize('dtype', [np.int64, np.int16])
def test_word_matrix_form_equals_decode_sentence(dtype):
    rng = np.random.default_rng(11)
    S, V, EOS, PAD = 20, 50, 2, 0
    B = S + 1 + 8                                                   # EOS at every position 0 .. S - 1, absent, random
    # not the identity: dictionary ids 100 .. 247; word 7 is two BLEU words, word 9 none, the others one
    remap = np.stack(((rng.permutation(V) * 3 + 100), np.full(V, -1)), axis=1).astype(np.int32)
    remap[7, 1], remap[9] = 250, (-1, -1)
    words = rng.integers(3, V, size=(S, B))
    words[rng.integers(S, size=B), np.arange(B)] = PAD              # a PAD does not end a sentence
    for b in range(B):
        e = b if b <= S else int(rng.integers(0, S + 1))
        if e < S:
            words[e:, b] = rng.integers(0, V, size=S - e)           # (whatever a decode leaves behind the EOS)
            words[e, b] = EOS
    words[:, S] = np.arange(10, 10 + S)                             # no EOS and the two-word entry: S + 1 BLEU words
    words[5, S], words[1, 12], words[3, 15], words[4, 15] = 7, 9, 7, 7
    hyps = []
    for b in range(B):
        col = words[:, b].tolist()
        hyps.append([int(i) for w in (col[:col.index(EOS)] if EOS in col else col) for i in remap[w] if i >= 0])
    assert [len(h) for h in hyps[:3]] == [0, 1, 2] and len(hyps[S]) == S + 1 and 250 in hyps[15]
    pool = sorted(set(remap[:, 0].tolist()) - {-1})
    slots = rng.permutation(B).tolist()
    refs = [None] * B
    for b, h in enumerate(hyps):                                    # (references that share words with their hypothesis)
        refs[slots[b]] = [sentence(rng, int(rng.integers(1, 30)), pool[:8] + h[:6]) for _ in range(2)]
    slots[7] = slots[25] = -1
    corpus = se.caption_corpus(refs)
    status, out, err = launch(refs, corpus=corpus, words=words.astype(dtype), eos=EOS, remap=remap, slots=slots, n_dict=300)
    assert status == 0 and err == 0
    live = [(b, s) for b, s in enumerate(slots) if s >= 0]
    want = se.caption_parts_rows([refs[s] for _, s in live], [hyps[b] for b, _ in live], corpus)
    got = se._parts_of(out['hyp_len'][:B], out['lcs'][:B * 2].reshape(B, 2), out['dot'][:B * 8].reshape(B, 2, 4),
                       out['hnorm2'][:B * 4].reshape(B, 4))
    for (b, s), w in zip(live, want):
        compare(got[s], w)
    assert any(w['dot'][0][1] > 0 for w in want) and nothing_written(out, 0, 2)
    # a word outside the vocabulary, a remap entry outside the dictionary: err, and that slot is not written
    bad = words.copy()
    bad[0, 5] = V
    status, out, err = launch(refs, corpus=corpus, words=bad.astype(dtype), eos=EOS, remap=remap, n_dict=300)
    assert status == 0 and err == 1 and untouched(out['hyp_len'], [5], 1) and untouched(out['dot'], [5], 8)
    assert out['hyp_len'][6] == len(hyps[6])
    status, out, err = launch(refs, corpus=corpus, words=words.astype(dtype), eos=EOS, remap=remap, n_dict=int(remap.max()))
    assert status == 0 and err == 1 and untouched(out['hyp_len'], [15], 1)


def test_limits_refusals_and_fault_word():
    from speaker_follower_amd import _lib
    lib = _lib.lib
    assert se.bleu_limits() == (65536, 256, 512, 4)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sf_caption_scores(None, None, st) == _lib.SF_ERR_ARG
    rng = np.random.default_rng(3)
    alphabet = [0, 1, 2, 99]
    refs = [[sentence(rng, 12, alphabet), sentence(rng, 5, alphabet)] for _ in range(3)]
    hyps = [sentence(rng, 10, alphabet), sentence(rng, 9, alphabet), []]
    corpus = se.caption_corpus(refs)
    # above the compile-time limits: refused, nothing written, the fault word untouched
    for r, h, kw in (([[sentence(rng, 12, alphabet)] * 2] * 3, [sentence(rng, 257, alphabet)] + hyps[1:], {}),
                     ([[sentence(rng, 513, alphabet)] * 2] * 3, hyps, {}),
                     ([[[1]] * 5] * 3, hyps, {}),
                     (refs, hyps, dict(n_dict=65537))):
        status, out, err = launch(r, h, corpus, **kw)
        assert status == _lib.SF_ERR_UNSUPPORTED and nothing_written(out, 3, len(r[0])) and err == 0
    lib.sf_debug_bleu_limits(100, 10, 12, 2)
    try:
        check(refs, hyps, corpus=corpus, n_dict=100)                # just inside every limit
        for kw, r, h in ((dict(n_dict=101), refs, hyps),
                         (dict(n_dict=100), refs, [sentence(rng, 11, alphabet)] + hyps[1:]),
                         (dict(n_dict=100), [[sentence(rng, 13, alphabet), [1]]] * 3, hyps),
                         (dict(n_dict=100), [[[1], [2], [0]]] * 3, hyps)):
            status, out, err = launch(r, h, corpus, **kw)
            assert status == _lib.SF_ERR_UNSUPPORTED and nothing_written(out, 3, len(r[0])) and err == 0, kw
        # host copies that understate the lengths: the kernel sees the real ones, writes nothing for them, raises err
        status, out, err = launch(refs, [sentence(rng, 11, alphabet)] + hyps[1:], corpus, n_dict=100, max_hyp=10)
        assert status == 0 and err == 1 and untouched(out['hyp_len'], [0], 1) and untouched(out['hnorm2'], [0], 4)
        assert out['hyp_len'][1] == 9
        # score_results with most paths above the lowered limits: the host's numbers through the merge
        case = FX['sets'][0]
        host = evaluate(case, 3, device='cpu')
        lib.sf_debug_bleu_limits(0, 25, 40, 0)
        ev = evaluate(case, 3, device=DEV)
        assert 0 < len(ev.captions['on_host']) < 260 and ev.captions['on_host'] == ev.counts['on_host']
        same_captions(ev, host)
        lib.sf_debug_bleu_limits(300, 0, 0, 0)                      # the tables do not fit: everything on the host
        ev = evaluate(case, 3, device=DEV)
        assert len(ev.captions['on_host']) == 260 and ev.captions['cider_d'] == host.captions['cider_d']
    finally:
        lib.sf_debug_bleu_limits(0, 0, 0, 0)
    assert se.bleu_limits() == (65536, 256, 512, 4)
    # a slot outside its array, an id outside the dictionary: err[0], nothing written for that hypothesis
    for slots in ([0, 3, 2], [0, -2, 2]):
        status, out, err = launch(refs, hyps, corpus, slots=slots)
        assert status == 0 and err == 1 and untouched(out['lcs'], [1], 2) and out['hyp_len'][0] == 10
    status, out, err = launch([[[99, 1, 2], [0]]] * 3, hyps, corpus, n_dict=99)
    assert status == 0 and err == 1 and nothing_written(out, 3, 2)
    status, out, err = launch(refs, [[0, -1, 2]] + hyps[1:], corpus)
    assert status == 0 and err == 1 and untouched(out['dot'], [0], 8) and out['hyp_len'][1] == 9


# ------------------------------------------------------------------------------------------ score_results
def evaluate(case, ipp, device):
    ev = se.SpeakerEvaluation(items=FX['items'], splits=['sub_val_seen'], instructions_per_path=ipp, device=device,
                              caption_metrics=True)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        ev.summary, _ = ev.score_results(cases.build_results(FX['items'], case))
    return ev


def same_captions(ev, host):
    """An evaluator that formed parts on the device against the all-host one."""
    assert list(ev.summary) == list(host.summary) == BLEU_KEYS + ['rouge_l', 'cider_d']
    assert list(ev.captions['parts']) == list(host.captions['parts'])
    static = ev._caption_static()['static']
    for pid, want in host.captions['parts'].items():
        compare(ev.captions['parts'][pid], want, static[pid])
        assert ev.captions['rouge_l'][pid] == host.captions['rouge_l'][pid], pid
        assert abs(ev.captions['cider_d'][pid] - host.captions['cider_d'][pid]) <= TOL, pid
    for k in BLEU_KEYS[1:] + ['rouge_l']:
        assert ev.summary[k] == host.summary[k], k
    assert abs(ev.summary['cider_d'] - host.summary['cider_d']) <= TOL


@pytest.mark.parametrize('ipp', [1, 3])
@pytest.mark.parametrize('name', [c['name'] for c in FX['sets']])
def test_score_results_on_the_device_equals_the_host(name, ipp):
    case = next(c for c in FX['sets'] if c['name'] == name)
    ev, host = evaluate(case, ipp, DEV), evaluate(case, ipp, 'cpu')
    assert ev.captions['on_host'] == [] and len(host.captions['on_host']) == 260 == len(ev.captions['parts'])
    same_captions(ev, host)


# ------------------------------------------------------------------------------------------ score_speaker
@pytest.fixture(scope='module')
def speaker_world():
    return world.build_speaker_world()


def calls_during(fn):
    """fn() with the names of the library entries issued through _lib.call recorded."""
    from speaker_follower_amd import _lib
    names, call = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)
    _lib.call = recording
    try:
        return fn(), names
    finally:
        _lib.call = call


def test_score_speaker_with_caption_metrics_equals_test_plus_score_results(speaker_world):
    w = speaker_world
    spk, env = w['spk'], w['env']
    ev = se.SpeakerEvaluation(env=env, device=DEV, caption_metrics=True)
    host = se.SpeakerEvaluation(env=env, device='cpu', caption_metrics=True)
    rewind = world.Rewind(env)
    results = spk.test(use_dropout=False, feedback='argmax')
    ev.summary, _ = ev.score_results(results)
    host.summary, _ = host.score_results(results)
    assert ev.captions['on_host'] == [] and len(host.captions['parts']) == 30
    same_captions(ev, host)
    by_results = dict(ev.captions)
    losses = list(spk.losses)
    end = rewind.after()
    rewind()
    sweeps = ev.sweeps
    (got, nothing), names = calls_during(lambda: ev.score_speaker(spk))
    assert rewind.after() == end                                    # env.ix, the item order, the next random.random()
    assert nothing is None and spk.results == {}
    assert ev.last_host_syncs == 1 and ev.fallbacks == 0 and ev.sweeps == sweeps + 1
    assert names.count('sf_bleu_counts') == 6 == names.count('sf_caption_scores')
    print('score_speaker: %s; hypothesis lengths %s' % (got, sorted({p['hyp_len'] for p in ev.captions['parts'].values()})))
    ev.summary = got
    same_captions(ev, host)
    assert got['model_score'] == host.summary['model_score'] and spk.losses == losses
    # the sweep read the same words score_results was given
    for pid, parts in by_results['parts'].items():
        compare(ev.captions['parts'][pid], parts)
    lens = {p['hyp_len'] for p in ev.captions['parts'].values()}
    assert len(lens) > 1 and got['rouge_l'] > 0 and got['cider_d'] > 0
    assert all(ev.captions['parts'][pid]['hyp_len'] == ev.counts['rows'][pid][8] for pid in ev.counts['rows'])
    rewind()


def test_a_default_evaluators_sweep_is_unchanged(speaker_world):
    w = speaker_world
    spk, env, ev = w['spk'], w['env'], w['ev']
    on = se.SpeakerEvaluation(env=env, device=DEV, caption_metrics=True)
    rewind = world.Rewind(env)
    (got, _), names = calls_during(lambda: ev.score_speaker(spk))
    end = rewind.after()
    rewind()
    assert list(got) == BLEU_KEYS and ev.captions is None and ev._caption is None
    assert names.count('sf_bleu_counts') == 6 and 'sf_caption_scores' not in names
    assert ev.last_host_syncs == 1 and ev.fallbacks == 0
    assert not any(k.startswith('cap_') or k == 'tables' for t in ev._sweep_tables.values() if t for k in t)
    with_captions, _ = on.score_speaker(spk)
    assert rewind.after() == end
    rewind()
    for k in BLEU_KEYS:
        assert got[k] == with_captions[k], k
    assert sorted(ev.counts['rows']) == sorted(on.counts['rows'])
    assert all(ev.counts['rows'][p].tolist() == on.counts['rows'][p].tolist() for p in ev.counts['rows'])
    assert ev.counts['sums'].tolist() == on.counts['sums'].tolist()
