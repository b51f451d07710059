"""CPU: the numpy models and comparators of tests/mover_cases.py, before tests/test_gpu_movers.py trusts them.

  * the gather models equal oracle/np_env.py (panorama_feature, action_embedding) composed by hand, on every case
  * the dropout model equals oracle/rng.dropout_mask; the Adam model in float64 equals torch.optim.Adam in float64
  * every comparator refuses a planted error of the kind its kernels could make
  * the case tables reach every edge they are there for (asserted, so that a later edit cannot thin them)
"""
import numpy as np
import pytest

from oracle import np_env, rng as orng
from tests import mover_cases as MC

F32 = np.float32


def refuses(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)
    return True


# ------------------------------------------------------------------------------------------------ feature gathers
def reference_candidates(table, d, LOC, heading, elevation):
    """np_env.action_embedding per sample over its a_num real candidates (clamped views), zero-padded to A rows by
    np_env.action_variable; a sample at vp < 0 (a padded step) and one without candidates contribute zero rows."""
    B, A = d['cand_view'].shape
    V = table.shape[1]
    embs = []
    for b in range(B):
        n = int(d['a_num'][b]) if d['vp'][b] >= 0 else 0
        cv = np.clip(d['cand_view'][b, :n], 0, V - 1)
        embs.append(np_env.action_embedding(table[max(d['vp'][b], 0)], cv, heading[b, :n], elevation[b, :n], LOC)
                    if n else np.zeros((0, table.shape[2] + LOC), F32))
    U = np.zeros((B, A, table.shape[2] + LOC), F32)
    for b, e in enumerate(embs):
        U[b, :len(e)] = e
    return U


@pytest.mark.parametrize('case', MC.GATHER_CASES, ids=lambda c: 'V%d-I%d-L%d-A%d-B%d' % c)
def test_gather_models_equal_the_reference_lines(case):
    V, IMG, LOC, A, B = case
    assert LOC % 16 == 0
    rng = np.random.default_rng(list(case))
    heading, elevation = rng.uniform(-np.pi, np.pi, (B, A)), rng.uniform(-np.pi / 2, np.pi / 2, (B, A))
    d = MC.gather_inputs(case)
    d['sincos'] = MC.sincos_of_angles(heading, elevation)
    table = d['table16'].astype(F32)
    # panorama: env.py:773 per sample, zeros on a padded step
    X = MC.model_panorama(table, d['loc'], d['vp'], d['view'])
    for b in range(B):
        want = np_env.panorama_feature(table[d['vp'][b]], int(np.clip(d['view'][b], 0, V - 1)), d['loc']) \
            if d['vp'][b] >= 0 else np.zeros((V, IMG + LOC), F32)
        MC.same_bits(X[b], want.astype(F32), 'panorama row %d' % b)
    # candidates: env.py:60-75 + follower.py:300-320
    U, valid = MC.model_candidates(table, d['vp'], d['cand_view'], d['sincos'], d['a_num'], LOC)
    ref = reference_candidates(table, d, LOC, heading, elevation)
    MC.same_bits(U, ref, 'candidates')
    assert np.array_equal(valid, (np.arange(A)[None, :] < d['a_num'][:, None]).astype(F32))
    # single actions: speaker.py:104 `action_embedding[a]`, zeros for the stop action
    rows = MC.model_actions(table, d['vp'], d['cand_view'], d['sincos'], d['a_num'], d['act'], LOC)
    for b in range(B):
        a = int(d['act'][b])
        want = ref[b, min(a, A - 1)] if a > 0 else np.zeros(IMG + LOC, F32)
        MC.same_bits(rows[b], want, 'action row %d' % b)
    # path actions: speaker.py:87-104 over (step, path) pairs, through the two-candidate list of np_env.dense_speaker_inputs
    ld = IMG + LOC + 4
    out = MC.model_path_actions(table, d['vp'], d['path_view'], d['sincos'][:, A - 1], d['path_act'], LOC, MC.poison(B, ld))
    for b in range(B):
        if d['path_act'][b] > 0 and d['vp'][b] >= 0:
            want = np_env.action_embedding(table[d['vp'][b]], [0, int(np.clip(d['path_view'][b], 0, V - 1))],
                                           [0.0, heading[b, A - 1]], [0.0, elevation[b, A - 1]], LOC)[1]
        else:
            want = np.zeros(IMG + LOC, F32)
        MC.same_bits(out[b, :IMG + LOC], want, 'path action row %d' % b)
    assert MC.is_poison(out[:, IMG + LOC:]).all()


def test_gather_cases_cover_their_axes_and_edges():
    cases = MC.GATHER_CASES
    assert 20 <= len(cases) <= 28 and len(set(cases)) == len(cases)
    for axis, values in enumerate(((1, 3, 36), (4, 8, 64), (16, 32, 128), (1, 2, 16), (1, 5, 67))):
        seen = [c[axis] for c in cases]
        assert set(seen) == set(values) and all(seen.count(v) >= 2 for v in values), (axis, seen)
    edges = set().union(*(MC.gather_edges(c) for c in cases))
    want = {'vp<0', 'view<0', 'view>=V', 'cand_view<0', 'cand_view>=V', 'path_view<0', 'path_view>=V', 'a_num=0', 'a_num=1',
            'a_num=A', 'path_act<=0', 'path_act>0'} | {'act=' + a for a in MC.ACT_EDGES}
    assert edges >= want, want - edges
    assert set(MC.LD_OUT) == {'F', 'F+4', '2F'}
    V, IMG, LOC, A, B = MC.GATHER_BIG
    assert B * V * (IMG + LOC) // 4 > MC.GRID_PASS and B * (IMG + LOC) // 4 > MC.GRID_PASS       # every gather kernel
    assert MC.feature_table16(V, IMG).size <= 64
    assert 'vp<0' in MC.gather_edges(MC.GATHER_BIG) and 'view>=V' in MC.gather_edges(MC.GATHER_BIG)
    assert {loc for _, loc in MC.REFUSED_CAND_SHAPES} >= {4, 8, 24} and (6, 16) in MC.REFUSED_CAND_SHAPES
    assert all(img == 6 for img, _ in MC.REFUSED_PANO_SHAPES)


def test_table_elements_are_distinct_and_binary16():
    for V, IMG in {(c.V, c.IMG) for c in MC.GATHER_CASES}:
        t = MC.feature_table16(V, IMG)
        assert t.dtype == np.float16 and np.isfinite(t).all() and len(np.unique(t)) == t.size
        assert np.array_equal(t.astype(F32).astype(np.float16).view(np.uint16), t.view(np.uint16))
    s = MC.sincos_constants(67 * 16)
    assert len(np.unique(s)) == s.size
    loc = MC.location_table(36, 128)
    assert len(np.unique(loc)) == loc.size


def test_gather_comparator_refuses_planted_errors():
    case = MC.GatherCase(3, 8, 32, 16, 67)
    V, IMG, LOC, A, B = case
    d = MC.gather_inputs(case)
    table = d['table16'].astype(F32)
    U, _ = MC.model_candidates(table, d['vp'], d['cand_view'], d['sincos'], d['a_num'], LOC)
    # a swapped sin / cos group
    bad = U.copy()
    g = LOC // 4
    bad[:, :, IMG:IMG + g], bad[:, :, IMG + g:IMG + 2 * g] = U[:, :, IMG + g:IMG + 2 * g], U[:, :, IMG:IMG + g]
    assert refuses(MC.same_bits, bad, U)
    # the layout of four groups of max(LOC / 16, 1) float4 at LOC = 8: [s0 s0 s0 s0 s1 s1 s1 s1] for [s0 s0 s1 s1 s2 s2 s3 s3]
    sc = d['sincos'][:1, 1:2]
    want8 = MC._candidate_rows(table, d['vp'][:1] * 0, d['cand_view'][:1, 1:2] * 0, sc, 8)[0, 0, IMG:]
    assert np.array_equal(want8, np.repeat(sc[0, 0], 2))
    assert refuses(MC.same_bits, np.repeat(sc[0, 0, :2], 4), want8)
    # an unclamped view: the row of the neighbouring viewpoint (what index vp * V + view reads for view == V)
    over = np.argwhere((d['cand_view'] >= V) & (d['vp'] >= 0)[:, None] & (np.arange(A)[None, :] > 0) &
                       (np.arange(A)[None, :] < d['a_num'][:, None]))
    assert len(over)
    b, a = over[0]
    bad = U.copy()
    bad[b, a, :IMG] = table.reshape(-1, IMG)[(d['vp'][b] * V + d['cand_view'][b, a]) % (MC.N_VP * V)]
    assert refuses(MC.same_bits, bad, U)
    X = MC.model_panorama(table, d['loc'], d['vp'], d['view'])
    bad = X.copy()
    b = int(np.flatnonzero((d['view'] < 0) & (d['vp'] >= 0))[0])
    bad[b, :, IMG:] = d['loc'][1]                                     # (the clamped row is row 0)
    assert refuses(MC.same_bits, bad, X)
    # a vp < 0 row left non-zero (and the sign of a zero)
    b = int(np.flatnonzero(d['vp'] < 0)[0])
    bad = X.copy()
    bad[b, 0, 0] = table[0, 0, 0]
    assert refuses(MC.same_bits, bad, X)
    bad = X.copy()
    bad[b, 0, 0] = -0.0
    assert refuses(MC.same_bits, bad, X)
    # a clobbered padding column of the strided output
    ld = IMG + LOC + 4
    out = MC.model_actions(table, d['vp'], d['cand_view'], d['sincos'], d['a_num'], d['act'], LOC, MC.poison(B, ld))
    assert MC.is_poison(out[:, IMG + LOC:]).all() and not MC.is_poison(out[:, :IMG + LOC]).any()
    bad = out.copy()
    bad[B - 1, ld - 1] = 0.0
    assert refuses(MC.same_bits, bad, out)


# ----------------------------------------------------------------------------------------------------- row movers
def test_row_cases_cover_their_axes():
    cases = MC.ROW_CASES
    assert {c.w for c in cases} == set(MC.ROW_W) == {4, 8, 80, 512, 516} and {c.n for c in cases} == {1, 63, 257}
    assert {(c.lds - c.w, c.ldd - c.w) for c in cases} == {(0, 0), (0, 4), (4, 0), (4, 4)}
    assert {c.pattern for c in cases} == set(MC.ROW_PATTERNS)
    for w in MC.ROW_W:
        assert {c.lds - w for c in cases if c.w == w} == {0, 4} == {c.ldd - w for c in cases if c.w == w}
    first = last = neg = rep = False
    for c in cases:
        for scatter in (False, True):
            idx, pool = MC.row_indices(c, scatter)
            assert idx.shape == (c.n,) and idx.max() < pool and idx.min() >= -1
            live = idx[idx >= 0]
            if scatter:
                assert len(set(live.tolist())) == len(live), 'scatter indices must be distinct'
            else:
                rep = rep or len(set(live.tolist())) < len(live)
            first, last, neg = first or (idx == 0).any(), last or (idx == pool - 1).any(), neg or (idx < 0).all()
    assert first and last and neg and rep
    b = MC.ROW_BIG
    assert b.n == 2049 and b.w == 2052 and b.n * (b.w // 4) > MC.GRID_PASS
    assert [len(c.moves) for c in MC.MOVE_CASES].count(1) >= 1 and [len(c.moves) for c in MC.MOVE_CASES].count(4) >= 1
    assert MC.ROW_MOVES_MAX == 4
    for c in MC.MOVE_CASES:
        if len(c.moves) == 4:
            assert len({m[0] for m in c.moves}) == 4 and {m[3] for m in c.moves} == {0, 1}


def test_row_models_and_their_comparator():
    c = MC.RowCase(8, 5, 12, 12, 'perm')
    src = MC.counting(8, 12, 8)
    idx = np.asarray([3, -1, 0, 7, 3], np.int32)
    got = MC.model_gather_rows(src, idx, 8, MC.poison(6, 12))
    assert np.array_equal(got[0, :8], src[3, :8]) and not got[1, :8].any() and np.array_equal(got[4, :8], src[3, :8])
    assert MC.is_poison(got[:, 8:]).all() and MC.is_poison(got[5]).all()
    bad = got.copy()
    bad[1, 8] = 0.0                                                    # a zero row written one float4 too wide
    assert refuses(MC.same_bits, bad, got)
    sidx = np.asarray([5, -1, 0, 7, 2], np.int32)
    sc = MC.model_scatter_rows(src, sidx, 8, MC.poison(8, 12))
    assert np.array_equal(sc[5, :8], src[0, :8]) and np.array_equal(sc[2, :8], src[4, :8]) and MC.is_poison(sc[1]).all()
    assert MC.is_poison(sc[:, 8:]).all() and MC.is_poison(sc[[1, 3, 4, 6]]).all()
    bad = sc.copy()
    bad[1, :8] = src[1, :8]                                            # a skipped row (idx < 0) written all the same
    assert refuses(MC.same_bits, bad, sc)
    assert refuses(MC.model_scatter_rows, src, np.asarray([1, 1], np.int32), 8, MC.poison(8, 12))
    assert np.isnan(src[:, 8:]).all() and c.w == 8


# --------------------------------------------------------------------------------------------------- plain movers
def test_plain_mover_cases_and_comparators():
    assert MC.TRANSPOSE_CASES == [(1, 1), (1, 33), (31, 32), (32, 32), (33, 31), (64, 65), (100, 2176)]
    src = MC.counting(33, 31, 31)
    t = MC.model_transpose(src)
    assert t.shape == (31, 33) and t[5, 32] == src[32, 5]
    bad = t.copy()                                                     # the tile behind the row edge written at the column edge
    bad[:, 32] = 0.0
    bad[30, :] = src[:, 30][::-1]
    assert refuses(MC.same_bits, bad, t)
    assert set(MC.EMBED_CASES) == {(E, B) for E in (4, 32, 300) for B in (1, 100)}
    for E, B in MC.EMBED_CASES + [MC.EMBED_BIG]:
        idx = MC.embedding_indices(E, B)
        assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() == MC.EMBED_VOCAB - 1
        if B > 1:
            assert (idx == 0).any() and len(set(idx.tolist())) < B
    E, B = MC.EMBED_BIG
    assert B * (E // 4) > MC.GRID_PASS
    assert MC.FILL_N == (0, 1, 255, 256, 257, 1048577)
    assert {c.p for c in MC.DROP_CASES} == {0.0, 0.2, 0.5} and {c.N for c in MC.DROP_CASES} == {1, 300}
    assert {c.col0 for c in MC.DROP_CASES} == {0, 40} == {c.col0 for c in MC.DROP_CASES if c.p > 0}
    assert {c.row0 for c in MC.DROP_CASES} == {0, 17} == {c.row0 for c in MC.DROP_CASES if c.p > 0}
    assert all(len({c.lds, c.ldd, c.N}) == 3 and min(c.lds, c.ldd) > c.N for c in MC.DROP_CASES + [MC.DROP_BIG])
    assert MC.DROP_BIG.B * MC.DROP_BIG.N > MC.GRID_PASS


@pytest.mark.parametrize('case', MC.DROP_CASES, ids=lambda c: 'p%g-B%d-N%d-c%d-r%d' % (c.p, c.B, c.N, c.col0, c.row0))
def test_dropout_model_equals_the_oracle_mask(case):
    p, B, N, lds, ldd, col0, row0 = case
    src = -MC.counting(B, lds, N)                                      # negative: a dropped element must be +0
    out = MC.model_dropout_copy(src, case, MC.poison(B, ldd))
    full = orng.dropout_mask(MC.DROP_SEED, MC.DROP_STREAM, row0 + np.arange(B), col0 + N, float(F32(p)))
    m = full[:, col0:]
    assert set(np.unique(m).tolist()) <= {0.0, float(F32(1.0 / (1.0 - float(F32(p)))))}
    MC.same_bits(out[:, :N], (src[:, :N] * m) + F32(0.0), 'dropout')   # (x + 0 turns -0 into +0)
    assert MC.is_poison(out[:, N:]).all()
    if p == 0:
        MC.same_bits(out[:, :N], src[:, :N], 'pass-through')
    else:
        if B * N >= 300:
            assert 0 < (m == 0).mean() < 1
        shifted = MC.model_dropout_copy(src, case._replace(col0=col0 + 1), MC.poison(B, ldd))
        if B * N >= 300:                                               # the mask of the wrong column / the wrong row
            assert refuses(MC.same_bits, shifted, out)
            assert refuses(MC.same_bits, MC.model_dropout_copy(src, case._replace(row0=row0 + 1), MC.poison(B, ldd)), out)
    bad = out.copy()
    bad[0, N] = 0.0
    assert refuses(MC.same_bits, bad, out)


# ------------------------------------------------------------------------------------------------------- reducers
def test_reducer_cases_sit_on_the_unroll_remainders():
    assert MC.REDUCER_B == (1, 15, 16, 17, 48, 49, 64, 65, 193, 256, 257) and MC.REDUCER_D == (32, 64, 68)
    # dot_rows / colsum_prod: rows m = g, g + 16, ..; four-row unroll while m + 48 < M.  sum_accum: while m + 192 < M.
    assert any(B <= 48 for B in MC.REDUCER_B) and {49, 64, 65} <= set(MC.REDUCER_B)          # around the first unrolled pass
    assert {193, 256, 257} <= set(MC.REDUCER_B)                                              # around sum_accum's
    for B in MC.REDUCER_B:
        for D in MC.REDUCER_D:
            c = MC.reducer_case(B, D)
            assert c.wt.shape == (B, D) and (np.count_nonzero(c.wt, axis=1) == 1).all()
            assert all(np.all(c.g0[k] != 0) for k in c.g0)
            for k in c.grads:                                          # an accumulating gradient overwritten
                assert c.grads[k].shape == c.g0[k].shape
                assert refuses(MC.same_bits, c.grads[k] - c.g0[k], c.grads[k])
    c = MC.reducer_case(257, 68)
    f8 = np.float64
    # the same three sums by loops over rows, in another order
    b_a, b_out, w_out = c.g0['b_a'].astype(f8), c.g0['b_out'].astype(f8), c.g0['w_out'].astype(f8)
    for b in reversed(range(257)):
        dc = float(c.dlogit[b].astype(f8).sum())
        dr = (c.dlogit[b].astype(f8)[:, None] * c.U[b].astype(f8)).sum(0)
        dwt = c.w[2].astype(f8) @ dr + dc * c.w[3].astype(f8)
        b_a += dc * c.wt[b]
        b_out += dc
        w_out += dwt * c.t_a[b]
    MC.same_bits(b_a.astype(F32), c.grads['b_a'])
    MC.same_bits(b_out.astype(F32), c.grads['b_out'])
    MC.same_bits(w_out.astype(F32), c.grads['w_out'])


# ----------------------------------------------------------------------------------------------------------- Adam
def torch_adam(p, g, m, v, step, wd, dtype):
    """One step of torch.optim.Adam on the CPU in `dtype` from the given moments, as step number `step`."""
    import torch
    P = torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=dtype))
    P.grad = torch.tensor(np.asarray(g), dtype=dtype)
    opt = torch.optim.Adam([P], weight_decay=wd, **{'lr': MC.ADAM_HYPER['lr'], 'betas': (MC.ADAM_HYPER['beta1'], MC.ADAM_HYPER['beta2']),
                                                    'eps': MC.ADAM_HYPER['eps']})
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.tensor(np.asarray(m), dtype=dtype),
                        exp_avg_sq=torch.tensor(np.asarray(v), dtype=dtype))
    opt.step()
    st = opt.state[P]
    assert int(st['step']) == step
    return P.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()


@pytest.mark.parametrize('wd', MC.ADAM_WD)
@pytest.mark.parametrize('step', MC.ADAM_STEPS)
def test_adam_model_equals_torch_in_float64(step, wd):
    """Equal up to the last bits of float64 (4 ulps of the larger of the result and its operands: a fused multiply-add
    in either library may differ by one rounding) -- nine orders below the fp32 effects the GPU test weighs."""
    import torch
    assert MC.ADAM_N == (1, 2, 3, 4, 5, 7, 1023, 4194309) and MC.ADAM_STEPS == (1, 2, 1000) and MC.ADAM_WD == (0.0, 5e-4)
    assert (MC.ADAM_N[-1] >> 2) > MC.GRID_PASS and MC.ADAM_N[-1] % 4 == 1
    for n in (1, 7, 1023):
        p, g, m, v = MC.adam_state(n)
        if n >= 7:
            assert (g == 0).any() and (v == 0).any() and (np.sqrt(v[v > 0]) < 1e-9).any() and (np.sqrt(v) > 1e-3).any()
        got = MC.model_adam(p, g, m, v, step, wd)
        ref = torch_adam(p, g, m, v, step, wd, torch.float64)
        scale = np.max(np.abs(np.stack((p, g, m, v))), axis=0).astype(np.float64)         # (m + w (g - m) may cancel)
        for a, b, name in zip(got, ref, 'pmv'):
            assert np.all(np.abs(a - b) <= 4 * np.spacing(np.maximum(np.abs(b), scale))), (name, n, float(np.abs(a - b).max()))
    # consecutive steps 1, 2 from zero moments
    p, g, _, _ = MC.adam_state(1023, seed=1)
    P = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.Adam([P], lr=1e-4, weight_decay=wd)
    q, m, v = p.astype(np.float64), np.zeros(1023), np.zeros(1023)
    for s in (1, 2):
        P.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        q, m, v = MC.model_adam(q, g, m, v, s, wd)
        assert np.all(np.abs(q - P.detach().numpy()) <= 4 * np.spacing(np.abs(q)))


def test_adam_comparator_refuses_planted_errors():
    import torch
    n, step, wd = 1023, 2, 5e-4
    p, g, m, v = MC.adam_state(n)
    r = torch_adam(p, g, m, v, step, wd, torch.float64)
    f = torch_adam(p, g, m, v, step, wd, torch.float32)
    mine = MC.model_adam(p, g, m, v, step, wd, dtype=F32)
    for a, b, c, name in zip(mine, r, f, 'pmv'):
        e, e32, share = MC.adam_within(a, b, c, name)
        assert share <= 1.0
        if name == 'p':                                                # one step moves p by ~1e-4: the bound sees it
            assert 4 * e32 < 1e-5 and np.abs(np.asarray(b) - p).max() < 0.1
            moved = np.abs(np.asarray(b) - p)
            assert np.median(moved) > 2e-5
    for i in (0, 1, 3, 4, 5):                                          # one element of every class left unstepped
        bad = np.array(f[0])
        j = 6 * 20 + i
        bad[j] = p[j]
        assert refuses(MC.adam_within, bad, r[0], f[0]), i
    for k in range(3):                                                 # a tail element left unstepped
        bad = np.array(f[k])
        bad[n - 1] = (p, m, v)[k][n - 1]
        assert refuses(MC.adam_within, bad, r[k], f[k])
    bad = np.array(f[0])                                               # eps forgotten where v is zero: a step of lr * m / 0
    bad[np.flatnonzero(v == 0)[0]] = np.inf
    assert refuses(MC.adam_within, bad, r[0], f[0])
    no_wd = torch_adam(p, g, m, v, step, 0.0, torch.float32)           # the weight decay dropped
    assert refuses(MC.adam_within, no_wd[1], r[1], f[1])
    wrong_step = torch_adam(p, g, m, v, step + 1, wd, torch.float32)   # the bias correction of the wrong step
    assert refuses(MC.adam_within, wrong_step[0], r[0], f[0])
    c0, c1 = MC.adam_coef(3)
    assert c0.dtype == F32 and abs(float(c0) - 1e-4 / (1 - 0.9 ** 3)) < 1e-10 and abs(float(c1) - (1 - 0.999 ** 3) ** -0.5) < 1e-5
