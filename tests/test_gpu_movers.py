"""GPU: the kernels of csrc/sf_pointwise.hip that move data or step parameters, each alone through its C entry, against
the numpy models of tests/mover_cases.py (proved on the CPU by tests/test_mover_cases_host.py), at the edges their own
code draws: the 4096 x 256-item pass of the grid-stride loops, the sin/cos group boundaries of cand_load, clamped views
and negative viewpoints, n % 4 tails, the unroll remainders of the reducers, the 32 x 32 tile edge of the transpose.

    1  sf_gather_panorama / _candidates / _actions / _actions_ld / _path_actions     on an fp32 and on a binary16 table
    2  sf_gather_rows / sf_scatter_rows / sf_move_rows
    3  sf_transpose, sf_embedding_fwd, sf_fill_f32, sf_add_f32, sf_dropout_copy
    4  dot_rows_kernel, sum_accum_kernel, colsum_prod_kernel through sf_eltwise_prod_scoring_bwd
    5  sf_adam_step / sf_adam_step_dev

1 - 4 are copies, selects or sums of small integers and are compared BIT FOR BIT, poison included: whatever the contract
does not name must keep its bits.  Nothing is filtered or skipped.  Every test asserts from sf_profile_begin /
sf_profile_end which kernels ran (the `<f16>` instantiation for a table registered with sf_feature_table_f16), and the
refusals of include/sf_hip.h (LOC in {4, 8, 24}, IMG = 6 in index form) assert the status, an empty profile and an
untouched output.  The NULL-pointer checks of sf_gather_actions / _ld and the n > INT_MAX check of sf_add_f32 are
verified by reading only: a test of them would be a deliberate fault on a library without the check.

Adam follows the rule of tests/grad_compare.py: with r = torch.optim.Adam in float64 on the CPU and f the same in
float32, each of p, m, v must satisfy |got - r| <= max(4 max|f - r|, two fp32 ulps of |r|) elementwise.  Every case
prints e = max|got - r| and e32 = max|f - r| (pytest -s).  The product n x weight decay x step is run whole for the
small n; n = 4 194 309 (one float4 pass plus one, tail 1) runs at (wd 5e-4, step 2) and (wd 0, step 1000).

Out of scope: the encoder-side movers reverse_tokens, bi_assemble, bi_split, dropout_tm, dropout_steps, ctx_grad_slice
and embedding_bwd have no C entry of their own; they are reached through the encoder entries only
(tests/test_gpu_bidirectional.py, tests/test_gpu_lstm_steps.py, tests/test_gpu_trainable_embeddings.py).

Found: the kernels themselves moved every bit right.  Wrong were three entry contracts, fixed with this module:
  * cand_load's four groups of max(LOC / 16, 1) float4 are the reference's LOC / 4 repeats only for LOC % 16 == 0, and
    (IMG + LOC) >> 2 drops columns of an fp32 table unless both are multiples of 4: sf_gather_candidates, sf_gather_actions,
    sf_gather_actions_ld and sf_follower_glue_fwd (index form) now refuse other shapes, sf_gather_panorama refuses
    IMG % 4 or LOC % 4, for both storages;
  * pano_row indexed the location table with the agent view unclamped (every other table index is clamped): view < 0 or
    >= V read outside the table.  It is clamped now, as include/sf_hip.h says;
  * sf_gather_actions / _ld did not check the pointers of sf_cands, sf_add_f32 narrowed its size_t n to int.

Measured on an MI355X (e = max|got - r|, e32 = max|f - r|; the share is the largest |got - r| / bound of any element):

    Adam p    e 2.37e-07, e32 2.37e-07 (n 4 194 309, wd 0, step 1000)      worst share of a bound 0.25
    Adam m    e 6.72e-08, e32 6.72e-08 (n 4 194 309, wd 5e-4, step 2)      worst share 0.25
    Adam v    e 1.97e-08, e32 1.97e-08 (n 4 194 309, wd 0, step 1000)      worst share 0.25

0.25 is the kernel landing on the float32 reference's own bits at the reference's worst element (|got - r| = |f - r|
against 4 |f - r|); no comparison of the 153 went above it.  One step moves p by ~1e-4 and the bound stays below 1e-6, so
an element left unstepped is a hundred bounds away.  coef[0..1] of sf_adam_step_dev equal the host's double computation
rounded once, bit for bit, at steps 1, 2 and 3.

The whole module (213 tests) takes 3.4 s of wall time (5.7 s with the interpreter's start); its slowest tests are the
first one (1.4 s: the library's first launch) and the 4 194 309-element Adam cases (0.2 .. 0.5 s).

Sensitivity, once on a scratch build with eight planted errors that change values only: cand_load's last group boundary
(`>= 3 g4` -> `> 3 g4`), the last element of the Adam tail unstepped, one row of colsum_prod's unrolled pass taken twice,
dot_rows' remainder loop one row short, sum_accum's fourth accumulator on the third's elements, gather_rows without its
grid stride, the transpose's last tile row not loaded, dropout_copy's col0 ignored.  131 of the 213 cases fail: 48 of 50
gather cases (the two that pass hold one row without candidates), every Adam case with a tail (40 of 46), 31 of 33
reducer cases, the one gather_rows case above a grid pass, all 7 transposes, the 4 dropout cases with p > 0 and col0 = 40.
"""
import contextlib
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mover_cases as MC                                   # noqa: E402

F32 = np.float32
ADAM_ROWS = []                              # (what, tensor, e, e32, share) of every Adam comparison of the session


def api():
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import ptr, stream, ws_args
    return _lib, ptr, stream, ws_args


def up(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()            # (a copy: the shared references are read-only)


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def profiled(fn):
    """fn() under the library's kernel profile, synchronised -> (its result, {kernel name: calls})."""
    _lib = api()[0]
    with _lib.kernel_profile() as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {k: v['calls'] for k, v in prof.rows.items()}


def run(expect, name, *args):
    """One call of entry `name` that must return SF_OK and launch exactly the kernels `expect` {name: calls}."""
    _lib = api()[0]
    _, rows = profiled(lambda: _lib.call(name, *args))
    assert rows == expect, '%s launched %s, expected %s' % (name, rows, expect)


def refused(status, name, *args):
    """One call that must return `status` and launch nothing."""
    _lib = api()[0]
    rc, rows = profiled(lambda: getattr(_lib.lib, name)(*args))
    assert rc == status and rows == {}, '%s: status %d (expected %d), launched %s' % (name, rc, status, rows)


@contextlib.contextmanager
def table_on_device(table16, storage):
    """The feature table as an fp32 or a binary16 device tensor, its storage registered with the library by address
    (and forgotten afterwards: the caching allocator hands addresses out again)."""
    _lib = api()[0]
    t = up(table16 if storage == 'fp16' else table16.astype(F32))
    addr = C.c_void_p(t.data_ptr())
    _lib.call('sf_feature_table_f16', addr, 1 if storage == 'fp16' else 0)
    assert _lib.lib.sf_feature_table_is_f16(addr) == (storage == 'fp16')
    try:
        yield t
    finally:
        torch.cuda.synchronize()
        _lib.call('sf_feature_table_f16', addr, 0)


def kname(kernel, storage):
    return kernel + ('<f16>' if storage == 'fp16' else '')


@pytest.fixture(scope='module', autouse=True)
def report():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    t0 = time.perf_counter()
    yield
    worst = {}
    for what, key, e, e32, share in ADAM_ROWS:
        if key not in worst or share > worst[key][0]:
            worst[key] = (share, what, e, e32)
    for key in sorted(worst):
        share, what, e, e32 = worst[key]
        print('[movers] adam worst of %s: (e, e32) = (%.2e, %.2e), share of the bound %.2f  [%s]' % (key, e, e32, share, what))
    print('[movers] module wall time %.1f s' % (time.perf_counter() - t0))


# ================================================================================================ 1. feature gathers
@functools.lru_cache(maxsize=None)
def gather_reference(case):
    """Inputs and every model output of one case, computed once and shared by the two storages (read-only)."""
    V, IMG, LOC, A, B = case
    d = MC.gather_inputs(case)
    t = d['table16'].astype(F32)
    F = IMG + LOC
    r = dict(d)
    r['pano'] = MC.model_panorama(t, d['loc'], d['vp'], d['view'])
    r['cand'], r['valid'] = MC.model_candidates(t, d['vp'], d['cand_view'], d['sincos'], d['a_num'], LOC)
    r['act_rows'] = MC.model_actions(t, d['vp'], d['cand_view'], d['sincos'], d['a_num'], d['act'], LOC)
    r['path'] = MC.model_path_actions(t, d['vp'], d['path_view'], d['path_sincos'], d['path_act'], LOC, MC.poison(B + 1, F + 4))
    for v in r.values():
        v.setflags(write=False)
    return r


GATHER_IDS = lambda c: 'V%d-I%d-L%d-A%d-B%d' % c                       # noqa: E731


@pytest.mark.parametrize('storage', ['fp32', 'fp16'])
@pytest.mark.parametrize('case', MC.GATHER_CASES + [MC.GATHER_BIG], ids=GATHER_IDS)
def test_feature_gathers_bit_for_bit(case, storage):
    """The five gather entries on one case: table rows (fp32, or binary16 widened exactly) beside location rows or
    sin/cos groups, zero rows for vp < 0 / stop / padding candidates / act <= 0, clamped view, cand_view and action
    indices, is_valid, strided outputs whose padding columns keep their poison."""
    _lib, ptr, stream, _ = api()
    V, IMG, LOC, A, B = case
    F = IMG + LOC
    r = gather_reference(case)
    dev = {k: up(r[k]) for k in ('loc', 'vp', 'view', 'cand_view', 'sincos', 'a_num', 'act', 'path_view', 'path_sincos', 'path_act')}
    with table_on_device(r['table16'], storage) as table:
        pano = _lib.Pano(None, table.data_ptr(), dev['loc'].data_ptr(), dev['vp'].data_ptr(), dev['view'].data_ptr(), V, IMG, LOC)
        cands = _lib.Cands(None, table.data_ptr(), dev['vp'].data_ptr(), dev['cand_view'].data_ptr(), dev['sincos'].data_ptr(),
                           dev['a_num'].data_ptr(), A, V, IMG, LOC)
        what = '%s %s ' % (GATHER_IDS(case), storage)
        # (one row of poison behind every output: a kernel that runs past the end shows)
        out = up(MC.poison(B + 1, V, F))
        run({kname('gather_pano_kernel', storage): 1}, 'sf_gather_panorama', C.byref(pano), B, ptr(out), stream())
        got = down(out)
        MC.same_bits(got[:B], r['pano'], what + 'panorama')
        assert MC.is_poison(got[B]).all()

        all_u, valid = up(MC.poison(B + 1, A, F)), up(MC.poison(B + 1, A))
        run({kname('gather_cand_kernel', storage): 1}, 'sf_gather_candidates', C.byref(cands), B, ptr(all_u), ptr(valid), stream())
        got, gv = down(all_u), down(valid)
        MC.same_bits(got[:B], r['cand'], what + 'candidates')
        MC.same_bits(gv[:B], r['valid'], what + 'is_valid')
        assert MC.is_poison(got[B]).all() and MC.is_poison(gv[B]).all()
        all_u2 = up(MC.poison(B + 1, A, F))                            # is_valid is optional
        run({kname('gather_cand_kernel', storage): 1}, 'sf_gather_candidates', C.byref(cands), B, ptr(all_u2), None, stream())
        MC.same_bits(down(all_u2), got, what + 'candidates without is_valid')

        rows = up(MC.poison(B + 1, F))
        run({kname('gather_action_kernel', storage): 1}, 'sf_gather_actions', C.byref(cands), B, ptr(dev['act']), ptr(rows), stream())
        got = down(rows)
        MC.same_bits(got[:B], r['act_rows'], what + 'actions')
        assert MC.is_poison(got[B]).all()
        for kind in MC.LD_OUT:
            ld = MC.ld_out(kind, F)
            host = MC.poison(B + 1, ld)
            rows = up(host)
            run({kname('gather_action_kernel', storage): 1}, 'sf_gather_actions_ld', C.byref(cands), B, ptr(dev['act']), ptr(rows),
                ld, stream())
            want = host.copy()
            want[:B, :F] = r['act_rows']
            MC.same_bits(down(rows), want, what + 'actions ld ' + kind)

        rows = up(MC.poison(B + 1, F + 4))
        run({kname('gather_path_actions_kernel', storage): 1}, 'sf_gather_path_actions', ptr(table), V, IMG, LOC, ptr(dev['vp']),
            ptr(dev['path_view']), ptr(dev['path_sincos']), ptr(dev['path_act']), B, ptr(rows), F + 4, stream())
        MC.same_bits(down(rows), r['path'], what + 'path actions')


@pytest.mark.parametrize('storage', ['fp32', 'fp16'])
@pytest.mark.parametrize('LOC', [4, 8, 24])
def test_panorama_takes_every_loc_multiple_of_four(LOC, storage):
    """The panorama copies location rows and has no sin/cos groups: LOC % 4 == 0 is all it needs."""
    _lib, ptr, stream, _ = api()
    case = MC.GatherCase(3, 8, LOC, 2, 5)
    V, IMG, _, A, B = case
    d = MC.gather_inputs(case)
    want = MC.model_panorama(d['table16'].astype(F32), d['loc'], d['vp'], d['view'])
    loc, vp, view, out = up(d['loc']), up(d['vp']), up(d['view']), up(MC.poison(B + 1, V, IMG + LOC))
    with table_on_device(d['table16'], storage) as table:
        pano = _lib.Pano(None, table.data_ptr(), loc.data_ptr(), vp.data_ptr(), view.data_ptr(), V, IMG, LOC)
        run({kname('gather_pano_kernel', storage): 1}, 'sf_gather_panorama', C.byref(pano), B, ptr(out), stream())
    got = down(out)
    MC.same_bits(got[:B], want, 'panorama LOC %d' % LOC)
    assert MC.is_poison(got[B]).all()


@pytest.mark.parametrize('storage', ['fp32', 'fp16'])
@pytest.mark.parametrize('IMG,LOC', MC.REFUSED_CAND_SHAPES)
def test_candidate_entries_refuse_other_shapes(IMG, LOC, storage):
    """Index form outside IMG % 4 == 0 && LOC % 16 == 0: SF_ERR_UNSUPPORTED from sf_gather_candidates, sf_gather_actions,
    sf_gather_actions_ld and sf_follower_glue_fwd for both storages, nothing launched, every output untouched."""
    _lib, ptr, stream, _ = api()
    V, A, B = 3, 4, 5
    F = IMG + LOC
    rng = np.random.default_rng([IMG, LOC])
    table16 = MC.feature_table16(V, IMG)
    vp, cv = up(rng.integers(0, MC.N_VP, B).astype(np.int32)), up(rng.integers(0, V, (B, A)).astype(np.int32))
    sc, an, act = up(MC.sincos_constants(B * A)), up(np.full(B, A, np.int32)), up(np.ones(B, np.int32))
    UNS = _lib.SF_ERR_UNSUPPORTED
    with table_on_device(table16, storage) as table:
        cands = _lib.Cands(None, table.data_ptr(), vp.data_ptr(), cv.data_ptr(), sc.data_ptr(), an.data_ptr(), A, V, IMG, LOC)
        ld = (F + 7) & ~3
        all_u, valid, rows, rows_ld, u_next = (up(MC.poison(*s)) for s in ((B, A, F), (B, A), (B, F), (B, ld), (B, ld)))
        refused(UNS, 'sf_gather_candidates', C.byref(cands), B, ptr(all_u), ptr(valid), stream())
        refused(UNS, 'sf_gather_actions', C.byref(cands), B, ptr(act), ptr(rows), stream())
        refused(UNS, 'sf_gather_actions_ld', C.byref(cands), B, ptr(act), ptr(rows_ld), ld, stream())
        logit0 = rng.standard_normal((B, A)).astype(F32)
        logit, target, ended = up(logit0), up(np.ones(B, np.int64)), up(np.zeros(B, np.uint8))
        a_t, t_used = up(np.full(B, -7, np.int64)), up(np.full(B, -7, np.int64))
        score, ce, live = (up(MC.poison(B)) for _ in range(3))
        glue = _lib.FollowerGlue(None, target.data_ptr(), 1, ended.data_ptr(), a_t.data_ptr(), t_used.data_ptr(), score.data_ptr(),
                                 u_next.data_ptr(), ld, None, 0, ce.data_ptr(), live.data_ptr(), 0, 0, 0)
        refused(UNS, 'sf_follower_glue_fwd', C.byref(cands), B, ptr(logit), C.byref(glue), stream())
        for t in (all_u, valid, rows, rows_ld, u_next, score, ce, live):
            assert MC.is_poison(down(t)).all()
        assert np.array_equal(down(logit), logit0) and (down(a_t) == -7).all() and not down(ended).any()


@pytest.mark.parametrize('storage', ['fp32', 'fp16'])
@pytest.mark.parametrize('IMG,LOC', MC.REFUSED_PANO_SHAPES)
def test_panorama_refuses_other_shapes(IMG, LOC, storage):
    _lib, ptr, stream, _ = api()
    V, B = 3, 5
    table16 = MC.feature_table16(V, IMG)
    loc, vp, view = up(MC.location_table(V, LOC)), up(np.zeros(B, np.int32)), up(np.zeros(B, np.int32))
    out = up(MC.poison(B, V, IMG + LOC))
    with table_on_device(table16, storage) as table:
        pano = _lib.Pano(None, table.data_ptr(), loc.data_ptr(), vp.data_ptr(), view.data_ptr(), V, IMG, LOC)
        refused(_lib.SF_ERR_UNSUPPORTED, 'sf_gather_panorama', C.byref(pano), B, ptr(out), stream())
    assert MC.is_poison(down(out)).all()


# ==================================================================================================== 2. row movers
ROW_IDS = lambda c: 'w%d-n%d-lds%d-ldd%d-%s' % c                       # noqa: E731


@pytest.mark.parametrize('case', MC.ROW_CASES + [MC.ROW_BIG], ids=ROW_IDS)
def test_gather_and_scatter_rows_bit_for_bit(case):
    """dst[i, :w] = src[idx[i], :w] (idx < 0: zeros) and dst[idx[i], :w] = src[i, :w] (idx < 0: skipped): the padding
    columns of src hold NaN and are never read, everything of dst the contract does not name keeps its poison."""
    _, ptr, stream, _ = api()
    w, n, lds, ldd, pattern = case
    idx, pool = MC.row_indices(case, False)
    src, dst = MC.counting(pool, lds, w), MC.poison(n + 1, ldd)
    d_src, d_dst, d_idx = up(src), up(dst), up(idx)
    run({'gather_rows_kernel': 1}, 'sf_gather_rows', ptr(d_src), lds, ptr(d_idx), n, w, ptr(d_dst), ldd, stream())
    MC.same_bits(down(d_dst), MC.model_gather_rows(src, idx, w, dst), 'gather ' + ROW_IDS(case))
    MC.same_bits(down(d_src), src, 'gather source')
    idx, pool = MC.row_indices(case, True)
    src, dst = MC.counting(n, lds, w), MC.poison(pool + 1, ldd)
    d_src, d_dst, d_idx = up(src), up(dst), up(idx)
    run({'scatter_rows_kernel': 1}, 'sf_scatter_rows', ptr(d_src), lds, ptr(d_idx), n, w, ptr(d_dst), ldd, stream())
    MC.same_bits(down(d_dst), MC.model_scatter_rows(src, idx, w, dst), 'scatter ' + ROW_IDS(case))


@pytest.mark.parametrize('case', MC.MOVE_CASES, ids=lambda c: 'n%d-%dmoves' % (c.n, len(c.moves)))
def test_move_rows_bit_for_bit(case):
    """1 and SF_ROW_MOVES_MAX moves of different widths in one launch, gathers and scatters mixed: every move equals its
    separate model; the same struct with n = 0 returns SF_OK and launches nothing."""
    _lib, ptr, stream, _ = api()
    bufs = [MC.move_buffers(case, k) for k in range(len(case.moves))]
    dev = [(up(src), up(dst), up(idx)) for src, dst, idx, _, _ in bufs]
    moves = (_lib.RowMove * len(bufs))(*(
        _lib.RowMove(s.data_ptr(), d.data_ptr(), i.data_ptr(), case.moves[k][1], case.moves[k][2], case.moves[k][0], case.moves[k][3])
        for k, (s, d, i) in enumerate(dev)))
    run({}, 'sf_move_rows', moves, len(bufs), 0, stream())
    for k, (src, dst, idx, w, scatter) in enumerate(bufs):
        MC.same_bits(down(dev[k][1]), dst, 'n = 0, move %d' % k)
    run({'move_rows_kernel': 1}, 'sf_move_rows', moves, len(bufs), case.n, stream())
    for k, (src, dst, idx, w, scatter) in enumerate(bufs):
        model = MC.model_scatter_rows if scatter else MC.model_gather_rows
        MC.same_bits(down(dev[k][1]), model(src, idx, w, dst), 'move %d of %s' % (k, case.moves[k],))
        MC.same_bits(down(dev[k][0]), src, 'source of move %d' % k)


# =================================================================================================== 3. plain movers
@pytest.mark.parametrize('R,Cc', MC.TRANSPOSE_CASES)
def test_transpose_bit_for_bit(R, Cc):
    _, ptr, stream, _ = api()
    src = MC.counting(R, Cc, Cc)
    d_src, d_dst = up(src), up(MC.poison(Cc + 1, R))
    run({'transpose_kernel': 1}, 'sf_transpose', ptr(d_src), R, Cc, ptr(d_dst), stream())
    got = down(d_dst)
    MC.same_bits(got[:Cc], MC.model_transpose(src), 'transpose %d x %d' % (R, Cc))
    assert MC.is_poison(got[Cc]).all()


@pytest.mark.parametrize('E,B', MC.EMBED_CASES + [MC.EMBED_BIG])
def test_embedding_rows_bit_for_bit(E, B):
    _, ptr, stream, _ = api()
    table = MC.counting(MC.EMBED_VOCAB, E, E)
    idx = MC.embedding_indices(E, B)
    d_t, d_i, d_o = up(table), up(idx), up(MC.poison(B + 1, E))
    run({'embedding_rows_kernel': 1}, 'sf_embedding_fwd', ptr(d_t), E, ptr(d_i), B, ptr(d_o), stream())
    got = down(d_o)
    MC.same_bits(got[:B], MC.model_embedding(table, idx), 'embedding E %d B %d' % (E, B))
    assert MC.is_poison(got[B]).all()


@pytest.mark.parametrize('n', MC.FILL_N)
def test_fill_and_add_bit_for_bit(n):
    """sf_fill_f32 and sf_add_f32 (dst += src on small integers: exact); the element behind the end keeps its poison;
    n = 0 launches nothing."""
    _, ptr, stream, _ = api()
    host = MC.poison(n + 1)
    d = up(host)
    run({'fill_kernel': 1} if n else {}, 'sf_fill_f32', ptr(d), n, -2.5, stream())
    want = host.copy()
    want[:n] = -2.5
    MC.same_bits(down(d), want, 'fill n %d' % n)
    a = (np.arange(n + 1) % 1021 - 510).astype(F32)
    b = (np.arange(n + 1) % 509 * 3 - 700).astype(F32)
    a[n] = MC.poison(1)[0]
    d_a, d_b = up(a), up(b)
    _, rows = profiled(lambda: api()[0].call('sf_add_f32', ptr(d_a), ptr(d_b), n, stream()))
    assert (sorted(rows) == [] if n == 0 else len(rows) == 1 and next(iter(rows)).startswith('ew_kernel') and
            list(rows.values()) == [1]), rows
    want = a.copy()
    want[:n] = a[:n] + b[:n]
    MC.same_bits(down(d_a), want, 'add n %d' % n)
    MC.same_bits(down(d_b), b, 'add source')


@pytest.mark.parametrize('case', MC.DROP_CASES + [MC.DROP_BIG], ids=lambda c: 'p%g-B%d-N%d-c%d-r%d' % (c.p, c.B, c.N, c.col0, c.row0))
def test_dropout_copy_bit_for_bit(case):
    """dst[b, :N] = src[b, :N] x the mask of oracle/rng.dropout_mask at (global row row0 + b, column col0 + n): kept
    elements scaled by fp32 1 / (1 - p), dropped ones +0, p = 0 a plain copy; lds != ldd != N, padding untouched."""
    _lib, ptr, stream, _ = api()
    p, B, N, lds, ldd, col0, row0 = case
    src, dst = -MC.counting(B, lds, N), MC.poison(B + 1, ldd)
    d_src, d_dst = up(src), up(dst)
    drop = C.byref(_lib.Dropout(float(p), MC.DROP_SEED, row0, None, 1)) if p else None
    run({'dropout_copy_kernel': 1}, 'sf_dropout_copy', ptr(d_src), lds, B, N, ptr(d_dst), ldd, drop, MC.DROP_STREAM, col0, stream())
    want = dst.copy()
    want[:B] = MC.model_dropout_copy(src, case, dst[:B])
    MC.same_bits(down(d_dst), want, 'dropout')


# ======================================================================================= 4. scoring-backward reducers
@pytest.mark.parametrize('D', MC.REDUCER_D)
@pytest.mark.parametrize('B', MC.REDUCER_B)
def test_scoring_backward_small_parameter_gradients_bit_for_bit(B, D):
    """b_a += dc^T wt (dot_rows_kernel), b_out += sum dc (sum_accum_kernel), w_out += colsum(dwt * t_a)
    (colsum_prod_kernel) on sums of small integers, from non-zero exact starting values, at batch sizes on the unroll
    remainders (m + 48 < M, m + 192 < M)."""
    _lib, ptr, stream, ws_args = api()
    c = MC.reducer_case(B, D)
    A, F = MC.REDUCER_A, MC.REDUCER_F
    tw = [up(a) for a in c.w]
    sw = _lib.ScoringW(*(t.data_ptr() for t in tw), None, None)
    g = {k: up(v) for k, v in c.g0.items()}
    sg = _lib.ScoringW(None, None, None, g['b_a'].data_ptr(), g['w_out'].data_ptr(), g['b_out'].data_ptr(), None, None)
    U = up(c.U)
    cands = _lib.Cands(U.data_ptr(), None, None, None, None, None, A, 1, F, 0)
    h, wt, t_a, dl, dh = up(np.zeros((B, D), F32)), up(c.wt), up(c.t_a), up(c.dlogit), up(MC.poison(B, D))
    _, rows = profiled(lambda: _lib.call('sf_eltwise_prod_scoring_bwd', C.byref(sw), C.byref(sg), C.byref(cands), B, D, D, ptr(h),
                                         ptr(t_a), ptr(wt), ptr(dl), ptr(dh), *ws_args(h.device)))
    for k in ('dot_rows_kernel', 'sum_accum_kernel', 'colsum_prod_kernel'):
        assert rows.get(k) == 1, (k, rows)
    for k in ('b_a', 'b_out', 'w_out'):
        MC.same_bits(down(g[k]), c.grads[k], 'B %d D %d gradient of %s' % (B, D, k))
    assert not MC.is_poison(down(dh)).any()


# ============================================================================================================ 5. Adam
@functools.lru_cache(maxsize=2)
def adam_inputs(n):
    out = MC.adam_state(n)
    for a in out:
        a.setflags(write=False)
    return out


def torch_adam_steps(p, grads, m, v, first_step, wd, dtype):
    """torch.optim.Adam on the CPU in `dtype`: len(grads) consecutive steps starting as step number first_step from the
    moments (m, v) -> [(p, m, v) after each step]."""
    P = torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=dtype))
    h = MC.ADAM_HYPER
    opt = torch.optim.Adam([P], lr=h['lr'], betas=(h['beta1'], h['beta2']), eps=h['eps'], weight_decay=wd)
    opt.state[P] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=torch.tensor(np.asarray(m), dtype=dtype),
                        exp_avg_sq=torch.tensor(np.asarray(v), dtype=dtype))
    out = []
    for g in grads:
        P.grad = torch.tensor(np.asarray(g), dtype=dtype)
        opt.step()
        st = opt.state[P]
        out.append((P.detach().numpy().copy(), st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()))
    assert int(opt.state[P]['step']) == first_step + len(grads) - 1
    return out


def check_adam(what, got, r, f):
    for name, a, b, c in zip('pmv', got, r, f):
        e, e32, share = MC.adam_within(a, b, c, '%s %s' % (what, name))
        print('[movers] %-40s %s  e = %.2e  e32 = %.2e  share of the bound %.2f' % (what, name, e, e32, share))
        ADAM_ROWS.append((what, name, e, e32, share))


ADAM_CASES = [(n, wd, s) for n in MC.ADAM_N[:-1] for wd in MC.ADAM_WD for s in MC.ADAM_STEPS] + \
             [(MC.ADAM_N[-1], 5e-4, 2), (MC.ADAM_N[-1], 0.0, 1000)]


@pytest.mark.parametrize('n,wd,step', ADAM_CASES)
def test_adam_step_within_the_fp32_reference_error(n, wd, step):
    """sf_adam_step as step number `step` from given moments: exact zeros in the gradient, v at and near zero (eps decides
    the quotient), the n % 4 tail, one float4 grid pass plus one.  The gradient is read only; one poisoned element
    behind every buffer survives."""
    _lib, ptr, stream, _ = api()
    p, g, m, v = adam_inputs(n)
    h = MC.ADAM_HYPER
    r = torch_adam_steps(p, [g], m, v, step, wd, torch.float64)[0]
    f = torch_adam_steps(p, [g], m, v, step, wd, torch.float32)[0]
    tail = MC.poison(1)
    d = [up(np.concatenate((a, tail))) for a in (p, g, m, v)]
    run({'adam_kernel': 1}, 'sf_adam_step', ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), n, h['lr'], h['beta1'], h['beta2'], h['eps'],
        wd, step, stream())
    got = [down(t) for t in d]
    assert all(MC.is_poison(a[n:]).all() for a in got)
    MC.same_bits(got[1][:n], g, 'the gradient')
    check_adam('n %d wd %g step %d' % (n, wd, step), (got[0][:n], got[2][:n], got[3][:n]), r, f)


@pytest.mark.parametrize('wd', MC.ADAM_WD)
def test_adam_step_dev_counts_on_the_device(wd):
    """sf_adam_step_dev three times on one device counter (what three replays of a captured step do): steps 1, 2, 3 of
    torch.optim.Adam, the counter at 3, coef[0..1] the host's double computation rounded once; then a guarded call
    (skip_if_nonzero != 0): p, m, v and the counter keep their bits."""
    _lib, ptr, stream, _ = api()
    n = 1023
    p, _, _, _ = adam_inputs(n)
    rng = np.random.default_rng([n, 3])
    grads = [rng.standard_normal(n).astype(F32) * (np.arange(n) % 3 != 1) for _ in range(3)]
    zeros = np.zeros(n, F32)
    r = torch_adam_steps(p, grads, zeros, zeros, 1, wd, torch.float64)
    f = torch_adam_steps(p, grads, zeros, zeros, 1, wd, torch.float32)
    h = MC.ADAM_HYPER
    tail = MC.poison(1)
    d_p, d_m, d_v = (up(np.concatenate((a, tail))) for a in (p, zeros, zeros))
    counter, coef, guard = up(np.zeros(1, np.int32)), up(np.zeros(4, F32)), up(np.zeros(1, np.int32))

    def step(d_g, guard_word):
        run({'adam_coef_kernel': 1, 'adam_kernel': 1}, 'sf_adam_step_dev', ptr(d_p), ptr(d_g), ptr(d_m), ptr(d_v), n, h['lr'],
            h['beta1'], h['beta2'], h['eps'], wd, ptr(counter), ptr(coef), guard_word, stream())

    for s in range(3):
        step(up(grads[s]), None if s == 0 else ptr(guard))            # (a guard word that holds 0 changes nothing)
        got = [down(t) for t in (d_p, d_m, d_v)]
        assert all(MC.is_poison(a[n:]).all() for a in got)
        check_adam('dev wd %g step %d' % (wd, s + 1), [a[:n] for a in got], r[s], f[s])
        assert down(counter)[0] == s + 1
        c = down(coef)
        MC.same_bits(c[:2], np.asarray(MC.adam_coef(s + 1), F32), 'coef at step %d' % (s + 1))
        assert c[2] == 0.0
    before = [down(t).copy() for t in (d_p, d_m, d_v, counter)]
    guard.fill_(7)
    step(up(grads[0]), ptr(guard))
    for a, t, name in zip(before, (d_p, d_m, d_v, counter), ('p', 'm', 'v', 'counter')):
        MC.same_bits(down(t), a, 'guarded step: ' + name)
    assert down(coef)[2] == 1.0
