"""Every branch of the GEMM dispatch of csrc/sf_gemm.hip (linear_nt, gemm_nn_ws, gemm_tn, colsum), one kernel at a time,
held to EXACT results at its tile edges, under row strides, with poisoned surroundings.

The entries are called directly (sf_linear_fwd, sf_linear_slabs_fwd, sf_linear_bwd): the ops.* wrappers cannot pass
strides.  Each case names the kernel it is meant to reach and asserts with _lib.kernel_profile() that it ran.

Exact families (tests/gemm_cases.py): selection operands (one +-2^e per reduction, the other operand with full 24-bit
mantissas) and small integers; compared with np.array_equal.  Every case runs contiguous and with row strides
`width + 4 j`, j in {1, 3}; the padding columns of every input and two rows behind its last row hold NaN, those of every
output a sentinel that must come back bit-identical (sf_hip.h: the entries read and write nothing outside the operands).

Float64 family: one dense, badly scaled, asymmetric product per kernel family with act 0 and 1; the normalised error
e = max |got - ref64| / (|x| |W|^T + |b|) is held to max(4 e_ref32, 2^-22), e_ref32 being the same figure of numpy's
float32 product of the same operands (the factor 4: another summation order; the floor: the project's 2.5e-7 ceiling for
this quantity at its deepest reduction); with tanh, plus 4 x the error of float32 np.tanh on the same pre-activations.
Measured (e, e_ref32) per kernel family on an MI355X, act 0 | act 1 (e_ref32 is that of the pre-activation); of the
backward cases the output of the kernel the case is about:
    nt_small     gemm_nt_small_kernel<2, 4>   (47, 2044, 300)    (8.4e-08, 3.2e-07) | (5.3e-08, 3.2e-07)
    nt_stream    gemm_nt_kernel<3>            (37, 20, 2372)     (4.9e-08, 5.8e-08) | (3.2e-08, 5.8e-08)
    nt_split     gemm_nt_split_kernel<5>      (70, 128, 2368)    (2.0e-08, 6.5e-08) | (1.0e-08, 6.5e-08)
    nt_tiled     gemm_nt_tiled_kernel<5>      (70, 128, 2368)    (4.0e-08, 6.5e-08) | (2.7e-08, 6.5e-08)
    nt_big       gemm_nt_big_kernel           (515, 130, 2324)   (1.1e-07, 7.6e-08) | (4.7e-08, 7.6e-08)
    nn           gemm_nn_kernel<7>, dx        (113, 256, 64)     (1.1e-07, 2.1e-07) | (7.7e-08, 2.3e-07)
    tn           gemm_tn_kernel, dW           (250, 2048, 300)   (1.4e-07, 3.0e-07) | (1.7e-07, 3.3e-07)
    tn_tiled     gemm_tn_tiled_kernel, dW     (4097, 128, 132)   (2.9e-08, 5.0e-08) | (3.7e-08, 5.7e-08)
    tn_split     gemm_tn_split_kernel, dW     (257, 384, 256)    (8.4e-08, 2.6e-07) | (1.2e-07, 3.1e-07)
    tn_many_row  transposes + nt_big, dW      (1028, 100, 300)   (3.4e-08, 1.1e-07) | (3.8e-08, 1.1e-07)
(the tanh term, 4 x the error of float32 np.tanh, was 2.3e-07 .. 2.4e-07 in every forward case; db through colsum_kernel
stayed at or below 4.4e-08 against e_ref32 >= 7.5e-08.)
Kernels that had to leave an exact family: none.  Every kernel of the dispatch is exact on both families, strided or not.

Two shapes first planned for gemm_nt_big_kernel do not reach it and were replaced, the assertion kept: the short-reduction
kernel comes first in linear_nt and takes (515, 130, 96) and (512, 64, 32) (gemm_nt_small_kernel<1, 2>; they stay in
the table under that name), so gemm_nt_big_kernel's thresholds are met at (515, 130, 2324), (512, 64, 2320) and
(512, 1040, 52) -- K >= 32 alone is not enough, the dispatch also asks for four chunks of 16 -- with (511, 64, 2320) as
the shape one row short.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_cases as G                                      # noqa: E402


@pytest.fixture(scope='module')
def sf():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import types
    from speaker_follower_amd import _lib, runtime
    return types.SimpleNamespace(lib=_lib.lib, call=_lib.call, profile=_lib.kernel_profile, ptr=runtime.ptr,
                                 ws_args=runtime.ws_args, workspace=runtime.workspace)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def check_profile(rows, must, must_not=(), what=''):
    for name in must:
        assert name in rows, '%s: %s was not launched; launched: %s' % (what, name, sorted(rows))
    for name in must_not:
        assert name not in rows, '%s: %s was launched; launched: %s' % (what, name, sorted(rows))


def fwd_id(c):
    return '%s-%dx%dx%d%s' % (c.kernels[0].replace('gemm_', '').replace('_kernel', '').replace(', ', '_'), c.M, c.N, c.K,
                              '-f32' if c.f32 else '')


# --------------------------------------------------------------------------------- forward, exact
@pytest.mark.parametrize('strided', [0, 1], ids=['contiguous', 'strided'])
@pytest.mark.parametrize('index', range(len(G.FORWARD)), ids=[fwd_id(c) for c in G.FORWARD])
def test_forward_is_exact(sf, index, strided):
    """sf_linear_fwd, act = 0: bit-for-bit the selection / int64 reference on the kernel the case names; nothing outside
    [M, N] of y is written, nothing outside [M, K] of x enters a result."""
    c = G.FORWARD[index]
    M, N, K = c.M, c.N, c.K
    jx, _ = G.pads(strided, index)
    ldx, ldy = K + 4 * jx, N + 4 * strided
    for family in G.FWD_FAMILIES:
        what = '%s (%d,%d,%d) %s ldx=%d ldy=%d' % (c.kernels[0], M, N, K, family, ldx, ldy)
        inp = G.forward_inputs(family, M, N, [K])
        x, w = dev(G.layout(inp.x[0], ldx)), dev(G.layout(inp.w[0]))
        b = dev(G.layout(inp.b)) if inp.b is not None else None
        y = dev(G.layout(np.full((M, N), G.SENTINEL, np.float32), ldy, fill=G.SENTINEL))
        sf.lib.sf_debug_gate_product_f32(c.f32)
        try:
            with sf.profile() as prof:
                sf.call('sf_linear_fwd', sf.ptr(x), ldx, sf.ptr(w), sf.ptr(b), M, N, K, 0, sf.ptr(y), ldy,
                        *sf.ws_args(x.device))
            torch.cuda.synchronize()
        finally:
            sf.lib.sf_debug_gate_product_f32(0)
        check_profile(prof.rows, c.kernels, c.absent, what)
        got = host(y)
        bad = np.argwhere(got[:M, :N] != inp.ref)
        assert np.array_equal(got[:M, :N], inp.ref), '%s: %d wrong elements, first at %s: got %r, want %r' % (
            what, len(bad), bad[0], got[tuple(bad[0])], inp.ref[tuple(bad[0])])
        assert G.outside_is_untouched(got, M, N), what + ': wrote outside [M, N] of y'


# ------------------------------------------------------------------------------ two segments, raw slabs
@pytest.mark.parametrize('strided', [0, 1], ids=['contiguous', 'strided'])
@pytest.mark.parametrize('index', range(len(G.SLABS)),
                         ids=['%s-%dx%dx%d+%d' % (c.kernels[0], c.M, c.N, c.K1, c.K2) for c in G.SLABS])
def test_two_segment_slabs_sum_to_the_exact_product(sf, index, strided):
    """sf_linear_slabs_fwd over two reduction segments (a segment boundary inside a K split; a partial chunk in the middle
    of the reduction): the raw slabs, added up in float64 on the host, are the exact product."""
    c = G.SLABS[index]
    M, N, K1, K2 = c.M, c.N, c.K1, c.K2
    jx, jh = G.pads(strided, index)
    ldx, ldh = K1 + 4 * jx, K2 + 4 * jh
    for family in G.FWD_FAMILIES:
        what = '%s (%d,%d,%d+%d) %s ldx=%d ldh=%d' % (c.kernels[0], M, N, K1, K2, family, ldx, ldh)
        inp = G.forward_inputs(family, M, N, [K1, K2])
        x, h = dev(G.layout(inp.x[0], ldx)), dev(G.layout(inp.x[1], ldh))
        w, u = dev(G.layout(inp.w[0])), dev(G.layout(inp.w[1]))
        ks = C.c_int(0)
        with sf.profile() as prof:
            sf.call('sf_linear_slabs_fwd', sf.ptr(x), ldx, sf.ptr(w), K1, sf.ptr(h), ldh, sf.ptr(u), K2, M, N,
                    C.byref(ks), *sf.ws_args(x.device))
        torch.cuda.synchronize()
        check_profile(prof.rows, c.kernels, (G.REDUCE,), what)
        assert ks.value > 1, what                        # (the cases are about boundaries INSIDE a split)
        slabs = host(sf.workspace(x.device)[:ks.value * M * N * 4].view(torch.float32).view(ks.value, M, N))
        got = slabs.astype(np.float64).sum(0)
        ref = inp.ref.astype(np.float64) - (inp.b.astype(np.float64)[None, :] if inp.b is not None else 0.0)
        assert np.array_equal(got, ref), '%s: %d wrong elements of %d slabs' % (what, int((got != ref).sum()), ks.value)


# -------------------------------------------------------------------------------- backward, exact
def bwd_id(c):
    launched = [k for k, n in c.kernels if n > 0 and k.startswith('gemm_')]
    nn = [k for k in launched if k.startswith('gemm_nn')]
    name = (nn[0] if nn else launched[0]).replace('gemm_', '').replace('_kernel', '')
    return '%s-%dx%dx%d%s' % (name, c.M, c.N, c.K, '-acc' if c.accumulate_dx else '')


def run_bwd(sf, inp, M, N, K, act, accumulate_dx, lds, y=None, tn_rows=-1, f32=0):
    """One sf_linear_bwd call on `layout` buffers; returns (profile rows, dx, dw, db buffers on the host)."""
    ldx, ldy, lddy, lddx = lds
    x, w, dy = dev(G.layout(inp.x, ldx)), dev(G.layout(inp.w)), dev(G.layout(inp.dy, lddy))
    yb = dev(G.layout(y if y is not None else np.full((M, N), np.nan, np.float32), ldy))
    want_dx = inp.dx is not None
    dx0 = inp.dx0 if accumulate_dx else np.full((M, K), G.SENTINEL, np.float32)
    dx = dev(G.layout(dx0, lddx, fill=G.SENTINEL)) if want_dx else None
    dw = dev(G.layout(inp.dw0, fill=G.SENTINEL))
    db = dev(G.layout(inp.db0, fill=G.SENTINEL)) if inp.db is not None else None
    sf.lib.sf_debug_tn_split_min_rows(tn_rows)
    sf.lib.sf_debug_gate_product_f32(f32)
    try:
        with sf.profile() as prof:
            sf.call('sf_linear_bwd', sf.ptr(x), ldx, sf.ptr(w), sf.ptr(yb), ldy, sf.ptr(dy), lddy, M, N, K, act,
                    sf.ptr(dx), lddx, accumulate_dx, sf.ptr(dw), sf.ptr(db), *sf.ws_args(x.device))
        torch.cuda.synchronize()
    finally:
        sf.lib.sf_debug_tn_split_min_rows(-1)
        sf.lib.sf_debug_gate_product_f32(0)
    return prof.rows, (host(dx) if want_dx else None), host(dw), (host(db) if db is not None else None)


def assert_exact(got, ref, what):
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), '%s: %d wrong elements, first at %s: got %r, want %r' % (
        what, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize('strided', [0, 1], ids=['contiguous', 'strided'])
@pytest.mark.parametrize('index', range(len(G.BACKWARD)), ids=[bwd_id(c) for c in G.BACKWARD])
def test_backward_is_exact(sf, index, strided):
    """sf_linear_bwd, act = 0: dx (overwritten or added to), dW and db (added to non-zero integers) bit-for-bit the
    references, on the kernels the case names; the saved output y (not needed without tanh) is all NaN."""
    c = G.BACKWARD[index]
    M, N, K = c.M, c.N, c.K
    jx, jy = G.pads(strided, index)
    lds = (K + 4 * jx, N + 4 * strided, N + 4 * jy, K + 4 * jy)
    for family in G.BWD_FAMILIES:
        what = '%s (%d,%d,%d) %s acc=%d ld=%s' % (bwd_id(c), M, N, K, family, c.accumulate_dx, lds)
        inp = G.backward_inputs(family, M, N, K, c.accumulate_dx)
        if not c.with_dx:
            inp = inp._replace(dx=None)
        rows, dx, dw, db = run_bwd(sf, inp, M, N, K, 0, c.accumulate_dx, lds, tn_rows=c.tn_split_min_rows)
        if family != 'selx':                              # (selx asks for dW alone: no dx and db launches)
            for name, n in c.kernels:
                calls = rows[name]['calls'] if name in rows else 0
                assert calls == n, '%s: %d launches of %s, expected %d; launched: %s' % (
                    what, calls, name, n, {k: v['calls'] for k, v in rows.items()})
        if inp.dx is not None:
            assert_exact(dx[:M, :K], inp.dx, what + ' dx')
            assert G.outside_is_untouched(dx, M, K), what + ': wrote outside [M, K] of dx'
        assert_exact(dw[:N, :K], inp.dw, what + ' dW')
        assert G.outside_is_untouched(dw, N, K), what + ': wrote behind dW'
        if inp.db is not None:
            assert_exact(db[:N], inp.db, what + ' db')
            assert G.outside_is_untouched(db, N, 0), what + ': wrote behind db'


# ----------------------------------------------------------------------------------- float64 family
def bound(e_ref32):
    return max(4.0 * e_ref32, 2.0 ** -22)


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('case', [c for c in G.DENSE if c.entry == 'fwd'], ids=lambda c: c.family)
def test_forward_accuracy_class(sf, case, act):
    c = case
    M, N, K = c.M, c.N, c.K
    x, w, b = G.dense_forward(M, N, K)
    f64 = np.float64
    pre = x.astype(f64) @ w.astype(f64).T + b
    mag = np.abs(x).astype(f64) @ np.abs(w).astype(f64).T + np.abs(b)
    e_ref32 = float((np.abs((x @ w.T + b).astype(f64) - pre) / mag).max())
    ldx, ldy = K + 4, N + 4
    xd, wd, bd = dev(G.layout(x, ldx)), dev(G.layout(w)), dev(G.layout(b))
    y = dev(G.layout(np.full((M, N), G.SENTINEL, np.float32), ldy, fill=G.SENTINEL))
    sf.lib.sf_debug_gate_product_f32(c.f32)
    try:
        with sf.profile() as prof:
            sf.call('sf_linear_fwd', sf.ptr(xd), ldx, sf.ptr(wd), sf.ptr(bd), M, N, K, act, sf.ptr(y), ldy,
                    *sf.ws_args(xd.device))
        torch.cuda.synchronize()
    finally:
        sf.lib.sf_debug_gate_product_f32(0)
    check_profile(prof.rows, (c.kernel,), what=c.family)
    got = host(y)
    assert G.outside_is_untouched(got, M, N)
    ref, t_err = pre, 0.0
    if act:
        p32 = pre.astype(np.float32)
        t_err = 4.0 * float(np.abs(np.tanh(p32).astype(f64) - np.tanh(p32.astype(f64))).max())
        ref = np.tanh(pre)
    e = float((np.maximum(np.abs(got[:M, :N].astype(f64) - ref) - t_err, 0.0) / mag).max())
    print('[%s act=%d (%d,%d,%d)] e = %.2e, e_ref32 = %.2e, bound %.2e, tanh term %.2e'
          % (c.family, act, M, N, K, e, e_ref32, bound(e_ref32), t_err))
    assert e <= bound(e_ref32)


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('case', [c for c in G.DENSE if c.entry == 'bwd'], ids=lambda c: c.family)
def test_backward_accuracy_class(sf, case, act):
    c = case
    M, N, K = c.M, c.N, c.K
    x, w, dy, dx0, dw0, db0 = G.dense_backward(M, N, K)
    f64 = np.float64
    y = np.tanh(np.random.default_rng(M + N).standard_normal((M, N))).astype(np.float32) if act else None
    dpre = dy.astype(f64) * ((1.0 - y.astype(f64) ** 2) if act else 1.0)
    dpre32 = (dy * (np.float32(1.0) - y * y)).astype(np.float32) if act else dy
    ref = dict(dx=dpre @ w.astype(f64), dw=dw0 + dpre.T @ x.astype(f64), db=db0 + dpre.sum(0))
    mag = dict(dx=np.abs(dpre) @ np.abs(w).astype(f64), dw=np.abs(dw0) + np.abs(dpre).T @ np.abs(x).astype(f64),
               db=np.abs(db0) + np.abs(dpre).sum(0))
    ref32 = dict(dx=dpre32 @ w, dw=dw0 + dpre32.T @ x, db=db0 + dpre32.sum(0, dtype=np.float32))
    inp = G.BwdInputs(x, w, dy, dx0, dw0, db0, ref['dx'], ref['dw'], ref['db'])
    lds = (K + 4, N + 4, N + 12, K + 12)
    rows, dx, dw, db = run_bwd(sf, inp, M, N, K, act, 0, lds, y=y, tn_rows=c.tn_split_min_rows)
    check_profile(rows, (c.kernel,), what=c.family)
    assert G.outside_is_untouched(dx, M, K) and G.outside_is_untouched(dw, N, K) and G.outside_is_untouched(db, N, 0)
    got = dict(dx=dx[:M, :K], dw=dw[:N, :K], db=db[:N])
    for name in ('dx', 'dw', 'db'):
        e_ref32 = float((np.abs(ref32[name].astype(f64) - ref[name]) / mag[name]).max())
        e = float((np.abs(got[name].astype(f64) - ref[name]) / mag[name]).max())
        print('[%s act=%d (%d,%d,%d) %s] e = %.2e, e_ref32 = %.2e, bound %.2e'
              % (c.family, act, M, N, K, name, e, e_ref32, bound(e_ref32)))
        assert e <= bound(e_ref32), name
