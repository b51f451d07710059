"""Host checks of tests/gemm_cases.py: the references the GPU module compares bit for bit must themselves be exact in
float32 -- whatever the order of the reduction -- and the case tables must name every kernel of the GEMM dispatch."""
import numpy as np
import pytest

from tests import gemm_cases as G


def f32_products(x, w):
    """x w^T in float32 three ways: natural order, reversed K order, and as 8 K slabs added up afterwards."""
    K = x.shape[1]
    yield 'natural', x @ w.T
    yield 'reversed', np.ascontiguousarray(x[:, ::-1]) @ np.ascontiguousarray(w[:, ::-1]).T
    cuts = [K * i // 8 for i in range(9)]
    slabs = [x[:, a:b] @ w[:, a:b].T for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    total = slabs[0]
    for s in slabs[1:]:
        total = total + s
    assert total.dtype == np.float32
    yield '8 slabs', total


def forward_shapes():
    seen = []
    for c in G.FORWARD:
        if (c.M, c.N, (c.K,)) not in seen:
            seen.append((c.M, c.N, (c.K,)))
    seen += [(c.M, c.N, (c.K1, c.K2)) for c in G.SLABS]
    return seen


def backward_shapes():
    seen = []
    for c in G.BACKWARD:
        if (c.M, c.N, c.K, c.accumulate_dx) not in seen:
            seen.append((c.M, c.N, c.K, c.accumulate_dx))
    return seen


@pytest.mark.parametrize('family', G.FWD_FAMILIES)
def test_forward_references_are_exact_in_float32(family):
    for M, N, Ks in forward_shapes():
        inp = G.forward_inputs(family, M, N, list(Ks))
        x, w = np.concatenate(inp.x, axis=1), np.concatenate(inp.w, axis=1)
        assert x.dtype == np.float32 and w.dtype == np.float32 and inp.ref.dtype == np.float32
        bias = inp.b[None, :] if inp.b is not None else np.float32(0.0)
        for order, y in f32_products(x, w):
            assert np.array_equal(y + bias, inp.ref), (family, M, N, Ks, order)


@pytest.mark.parametrize('family', G.BWD_FAMILIES)
def test_backward_references_are_exact_in_float32(family):
    for M, N, K, acc in backward_shapes():
        inp = G.backward_inputs(family, M, N, K, acc)
        for order, dw in f32_products(np.ascontiguousarray(inp.dy.T), np.ascontiguousarray(inp.x.T)):
            assert np.array_equal(inp.dw0 + dw, inp.dw), (family, 'dW', M, N, K, order)
        if inp.dx is not None:
            for order, dx in f32_products(inp.dy, np.ascontiguousarray(inp.w.T)):
                assert np.array_equal((inp.dx0 if acc else np.float32(0.0)) + dx, inp.dx), (family, 'dx', M, N, K, order)
        if inp.db is not None:
            for db in (inp.dy.sum(0, dtype=np.float32), inp.dy[::-1].sum(0, dtype=np.float32)):
                assert np.array_equal(inp.db0 + db, inp.db), (family, 'db', M, N, K)


def test_selection_operands_are_what_they_claim():
    rng = np.random.default_rng(0)
    x = G.full_mantissa(rng, 64, 300)
    assert (np.abs(x) >= 0.5).all() and (np.abs(x) < 2.0).all()
    mant = (np.abs(x.astype(np.float64)) * 2.0 ** 24).astype(np.int64)      # integers below 2^25
    low = np.where(np.abs(x) < 1.0, mant, mant // 2) & 0xff                  # the lowest of the three bf16 planes
    assert (low != 0).mean() > 0.98 and ((mant // np.where(np.abs(x) < 1.0, 1, 2)) & 1).mean() > 0.4
    for rows, K in ((16, 4), (2048, 300), (64, 2368), (20, 2372), (300, 128)):
        m, col, val = G.selection(rng, rows, K)
        assert ((m != 0).sum(1) == 1).all() and np.array_equal(m[np.arange(rows), col], val)
        assert set(np.abs(val)) <= {2.0 ** e for e in range(-3, 4)}
        assert len(set(col[:K])) == min(rows, K)                             # a coprime to K: all of K before a repeat
        if rows > 2 and K > 8:
            assert len(set(np.diff(col) % K)) == 1 and (np.diff(col) % K)[0] not in (0, 1, K - 1)


def test_integer_cases_stay_below_2_to_the_24():
    for M, N, Ks in forward_shapes():
        assert 64 * max(sum(Ks), M) + 8 < 2 ** 24
    for M, N, K, _ in backward_shapes():
        assert 64 * max(K, M, N) + 8 < 2 ** 24
    big = max(c.K for c in G.BACKWARD)
    assert big == 4352                                                       # the deepest case of the tables


def test_int_matmul_routes_agree():
    rng = np.random.default_rng(1)
    a, b = G.small_ints(rng, 300, 700), G.small_ints(rng, 700, 400)
    exact = a.astype(np.int64) @ b.astype(np.int64)
    assert np.array_equal(G.int_matmul(a, b), exact)                          # (above the int64 route's size limit)
    assert 300 * 700 * 400 > 1 << 26
    assert np.array_equal(G.int_matmul(a[:50], b), exact[:50])


def test_layout_poisons_what_is_not_the_operand():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    buf = G.layout(a, 8)
    assert buf.shape == (3 + G.TAIL_ROWS, 8) and np.array_equal(buf[:3, :4], a)
    assert np.isnan(buf[:3, 4:]).all() and np.isnan(buf[3:]).all()
    out = G.layout(a, 8, fill=G.SENTINEL)
    assert G.outside_is_untouched(out, 3, 4)
    for r, col in ((0, 4), (2, 7), (3, 0), (4, 7)):
        hit = out.copy()
        hit[r, col] = np.nextafter(G.SENTINEL, np.float32(0))                 # one bit off
        assert not G.outside_is_untouched(hit, 3, 4)
    vec = G.layout(np.ones(5, np.float32), fill=G.SENTINEL)
    assert vec.shape == (5 + G.TAIL_ROWS,) and G.outside_is_untouched(vec, 5, 0)
    assert G.pads(0, 3) == (0, 0) and {G.pads(1, 0), G.pads(1, 1)} == {(1, 3), (3, 1)}


def test_tables_name_every_kernel_of_the_dispatch():
    want = {'gemm_nt_small_kernel<%d, %d>' % mc for mc in
            ((1, 2), (1, 4), (1, 8), (1, 16), (1, 18), (2, 2), (2, 4), (2, 8), (4, 2), (4, 4))}
    want |= {'gemm_nt_kernel<%d>' % m for m in range(1, 9)}
    want |= {'gemm_nt_split_kernel<%d>' % m for m in range(1, 9)}
    want |= {'gemm_nt_tiled_kernel<%d>' % m for m in range(1, 9)}
    want |= {'gemm_nn_kernel<%d>' % m for m in (1, 2, 4, 7)}
    want |= {'gemm_nt_big_kernel', 'gemm_tn_kernel', 'gemm_tn_tiled_kernel', 'gemm_tn_split_kernel', 'reduce_slabs_kernel',
             'colsum_kernel', 'colsum_finish_kernel', 'transpose_kernel'}
    assert G.named_kernels() == want
    # the float64 family: one case per kernel family, each naming a kernel of the tables
    assert {c.kernel for c in G.DENSE} <= want and len({c.family for c in G.DENSE}) == len(G.DENSE)
