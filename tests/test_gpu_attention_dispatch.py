"""The row-set kernels of csrc/sf_attention.hip -- visual attention, text attention, candidate scoring -- one kernel at a
time, at every edge of their dispatch and of their bodies (tests/attention_cases.py: the tables, the two input families,
the float64 references; tests/test_attention_cases_host.py checks those on the host).

The entries are called directly (the ops.* wrappers cannot pass strides); every case asserts with _lib.kernel_profile()
that the kernel it names ran, and that no other attention kernel did.  Strided vectors carry NaN in their padding columns
and in two rows behind the last (inputs) or a sentinel that must come back bit-identical (outputs).

Exact family (np.array_equal): the selection inputs -- one row outscores the rest by > 200, the softmax is one-hot, the
output is that row to the last bit; sample b designates row b mod V, cases listed with B = 3 run it with V (L) samples so
that every row of every wave and split group is designated.  The query / scoring vector is formed by the entry through
0 / 2^e weights and comes back exactly as built.  Backward: dyadic alpha, small-integer rows; one-hot dlogit.
What the entries do not return is read through 0 / 1 operands: dq = the rows of the W_v gradient under t_v = identity
(and dh = columns of dq), dr = the rows of the W_a gradient under wt = identity, dc = the b_a gradient.

Dense family: e = max |got - ref64| / max |ref64| against e32, the same figure of the float32 numpy evaluation of the same
formula on the inputs as the entry returned them (q, r, wt); e <= max(4 e32, 2e-6) and e <= 1e-4.  Measured on an MI355X
(the case with the largest e of each group as (e, e32); `-s` prints every figure):
    visual forward  un-split  visual_attn_kernel<0>        alpha (1.8e-07, 2.8e-07)   out (2.1e-07, 2.2e-07)
    visual forward  split     visual_attn_split_kernel     alpha (2.9e-07, 3.7e-07)   out (2.7e-07, 4.2e-07)
    visual forward  index form, fp32 = fp16 bits           alpha (3.1e-07, 2.3e-07)   out (3.7e-07, 3.4e-07)
    split merge, one group 60 below                        alpha (2.1e-06, 2.6e-06)   out (4.5e-07, 6.4e-07)
    visual backward           visual_attn_kernel<1>        dq    (4.9e-07, 1.8e-07)
    text forward              text_attn_kernel<1|5|8>      alpha (5.6e-07, 2.6e-07)   wc  (6.9e-07, 3.3e-07)
    text backward             text_attn_kernel<1|5|8>      dt    (1.0e-06, 5.5e-07)   dctx (3.9e-07, 4.9e-07)
    scoring forward           score_fwd_kernel             logit (2.1e-07, 4.9e-07)
    scoring backward          score_bwd_kernel             dr    (1.5e-07, 1.3e-07)   dc  (1.4e-07, 1.4e-07)
The float64-score forward (visual_attn_split_f64_kernel) is held to the bound of tests/test_gpu_precise.py: alpha within
1e-6, out within 5e-6 max(1, |out|) of the float64 evaluation from the float64 query (measured: alpha <= 9.9e-08, out <=
3.6e-06 at max |out| 20.7).  Every exact-family case passed bit for bit on every kernel: no kernel had to leave it.

Not reachable as planned, assertion kept under the planned name:
  * "fp16 flag with a dense source -> SF_ERR_ARG": the ABI never tags a dense source as half (sf_api_util.h: pano(), cands():
    `dense ? 0 : table_is_f16(table)`), so a sf_pano / sf_cands that names a registered binary16 table BESIDE a dense
    tensor runs the fp32 dense kernel on the dense rows; the test asserts that (same kernel name, same bits as without
    the table pointer) -- the table is never read as fp32.
  * ds directly: neither sf_text_attention_bwd nor sf_soft_dot_attention_bwd returns ds; the direct form is covered through
    dt and dctx (both are linear in ds), the deferred form by the follower passes below (ctx_grad_kernel consumes the ds
    the text kernel stored).

Deferred context gradient: follower teacher-forced training passes built as in tests/test_gpu_grads_f64.py (B = 3, float64
oracle, tests/grad_compare.py) with the longest instruction at 80 and 81 positions, and at 80 with 102 and 103 steps
(S L = 8160 | 8240 around the 8192 that fit ctx_grad_kernel's LDS).  ctx_grad_kernel must run exactly at (80, 102); the
context gradient -- every encoder gradient lies behind it -- matches the oracle in all three.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_model, rng as orng, torch_ref                  # noqa: E402
from speaker_follower_amd import synth                                # noqa: E402
from tests import attention_cases as AC                               # noqa: E402

TOL = dict(rtol=1e-4, atol=1e-4)
f64 = np.float64
SENT = AC.SENTINEL


@pytest.fixture(scope='module')
def sf():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from speaker_follower_amd import _lib, runtime, features
    return types.SimpleNamespace(L=_lib, call=_lib.call, profile=_lib.kernel_profile, ptr=runtime.ptr, ws_args=runtime.ws_args,
                                 stream=runtime.stream, dropout_arg=runtime.dropout_arg, features=features)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def sentinel(rows, cols, ld=None):
    return dev(AC.layout(np.full((rows, cols), SENT, np.float32), ld, fill=SENT))


def attention_kernels(rows):
    return sorted(k for k in rows if k.startswith(AC.ATTENTION_KERNELS))


def assert_ran(rows, kernel, what):
    """`kernel` ran once, and it is the only attention kernel of the call."""
    assert attention_kernels(rows) == [kernel], '%s: expected %s, launched %s' % (what, kernel, sorted(rows))
    assert rows[kernel]['calls'] == 1, (what, rows[kernel])


def assert_exact(got, ref, what):
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), '%s: %d wrong elements, first at %s: got %r, want %r' % (
        what, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def check_e(got, ref64, ref32, what):
    e, e32 = AC.rel_err(got, ref64), AC.rel_err(ref32, ref64)
    print('[%s] e = %.2e, e32 = %.2e, bound %.2e' % (what, e, e32, AC.bound(e32)))
    assert e <= AC.bound(e32), '%s: e = %.3e > bound %.3e (e32 = %.3e)' % (what, e, AC.bound(e32), e32)
    return e, e32


def one_hot(B, n, sel):
    a = np.zeros((B, n), np.float32)
    a[np.arange(B), sel] = 1.0
    return a


# ================================================================================================ visual attention
def visual_w(sf, w):
    tw = [dev(a) for a in (w.w_h, w.b_h, w.w_v, w.b_v)]
    tw += [tw[2].t().contiguous(), tw[0].t().contiguous()]
    return sf.L.VisualW(*(t.data_ptr() for t in tw)), tw


def dense_pano(sf, X):
    """A dense sf_pano over X [B, V, F], two NaN rows behind the last row of the last sample."""
    Xd = dev(AC.layout(X.reshape(-1, X.shape[2])))
    return sf.L.Pano(Xd.data_ptr(), None, None, None, None, X.shape[1], X.shape[2], 0), Xd


def run_visual_fwd(sf, pano, B, V, F, w, ldo=None, drop=None, stream=0, col0=0, entry='sf_visual_attention_fwd'):
    """-> (profile rows, out buffer [B + 2, ldo], alpha buffer [B + 2, V], t_v, q) on the host."""
    ldo = F + 4 if ldo is None else ldo
    H, D = w.h.shape[1], w.w_h.shape[0]
    vw, keep = visual_w(sf, w)
    h, out, alpha = dev(w.h), sentinel(B, F, ldo), sentinel(B, V)
    t_v, q = torch.empty(B, D, device='cuda'), torch.empty(B, F, device='cuda')
    with sf.profile() as prof:
        sf.call(entry, C.byref(vw), C.byref(pano), B, H, D, sf.ptr(h), sf.ptr(out), ldo, sf.ptr(alpha), sf.ptr(t_v),
                sf.ptr(q), drop, stream, col0, *sf.ws_args(h.device))
    torch.cuda.synchronize()
    return prof.rows, host(out), host(alpha), host(t_v), host(q)


def run_visual_bwd(sf, pano, B, V, F, alpha, dout, drop=None, stream=0, col0=0):
    """sf_visual_attention_bwd through the 0 / 1 weights of AC.copy_weights -> (rows, dq [B, F], dh [B, D], cols): dq is
    read from the W_v gradient (t_v = identity rows), dh = dq[:, cols]."""
    t_v, w_h, w_v, cols = AC.copy_weights(B, F)
    D = w_h.shape[0]
    tw = [dev(w_h), dev(np.zeros(D, np.float32)), dev(w_v), dev(np.zeros(D, np.float32))]
    vw = sf.L.VisualW(*(t.data_ptr() for t in tw), None, None)
    gwv = torch.zeros(D, F, device='cuda')
    vg = sf.L.VisualW(None, None, gwv.data_ptr(), None, None, None)
    lddo = F + 4
    h, al, tv, do = dev(np.zeros((B, D), np.float32)), dev(alpha), dev(t_v), dev(AC.layout(dout, lddo))
    dh = torch.zeros(B, D, device='cuda')
    with sf.profile() as prof:
        sf.call('sf_visual_attention_bwd', C.byref(vw), C.byref(vg), C.byref(pano), B, D, D, sf.ptr(h), sf.ptr(al),
                sf.ptr(tv), sf.ptr(do), lddo, drop, stream, col0, sf.ptr(dh), *sf.ws_args(h.device))
    torch.cuda.synchronize()
    gw = host(gwv)
    assert not gw[B:].any(), 'rows of the W_v gradient behind the batch must stay zero'
    return prof.rows, gw[:B], host(dh), cols


def vis_id(c):
    return '%s-V%d-B%d-F%d' % (c.kernel.replace('visual_attn_', '').replace('_kernel', ''), c.V, c.B, c.F)


def check_selection_forward(s, rows, out, alpha, q, kernel, what):
    B, V, F = s.X.shape
    assert_ran(rows, kernel, what)
    assert_exact(q, s.q, what + ' q (the 0 / 2^e weights must copy)')
    assert_exact(alpha[:B], one_hot(B, V, s.sel), what + ' alpha')
    assert_exact(out[:B, :F], s.X[np.arange(B), s.sel], what + ' out')
    assert AC.outside_is_untouched(out, B, F) and AC.outside_is_untouched(alpha, B, V), what + ': wrote outside out / alpha'


def check_dense_forward(X, rows, out, alpha, q, kernel, what):
    B, V, F = X.shape
    assert_ran(rows, kernel, what)
    a64, o64 = AC.visual_fwd(X, q)
    a32, o32 = AC.visual_fwd(X, q, np.float32)
    check_e(alpha[:B], a64, a32, what + ' alpha')
    check_e(out[:B, :F], o64, o32, what + ' out')
    assert AC.outside_is_untouched(out, B, F) and AC.outside_is_untouched(alpha, B, V), what + ': wrote outside out / alpha'


@pytest.mark.parametrize('case', AC.VISUAL, ids=vis_id)
def test_visual_forward_dense_source(sf, case):
    """sf_visual_attention_fwd on a dense panorama: both families, ldo = F + 4 (sentinel in the padding and behind out and
    alpha); the dense family also against np_model at the project's TOL."""
    c = case
    Bs = max(c.B, c.V) if c.B == 3 else c.B
    s = AC.visual_selection(Bs, c.V, c.F)
    pano, keep = dense_pano(sf, s.X)
    rows, out, alpha, t_v, q = run_visual_fwd(sf, pano, Bs, c.V, c.F, AC.visual_selection_weights(s))
    check_selection_forward(s, rows, out, alpha, q, c.kernel, vis_id(c) + ' selection')
    X, w = AC.visual_dense(c.B, c.V, c.F)
    pano, keep = dense_pano(sf, X)
    rows, out, alpha, t_v, q = run_visual_fwd(sf, pano, c.B, c.V, c.F, w)
    check_dense_forward(X, rows, out, alpha, q, c.kernel, vis_id(c) + ' dense')
    ref_out, ref_alpha = np_model.visual_soft_dot_attention(w.h, X, w.w_h, w.b_h, w.w_v, w.b_v)
    np.testing.assert_allclose(out[:c.B, :c.F], ref_out, **TOL)
    np.testing.assert_allclose(alpha[:c.B], ref_alpha, **TOL)


def index_inputs(B, V, IMG, LOC, X_img):
    """vp (one sample at -1, the others distinct and out of order), view, and the table that holds X_img[b] at row vp[b]."""
    vp = np.asarray([B - 1 - b if b != 1 else -1 for b in range(B)], np.int32)
    live = vp >= 0
    assert len(set(vp[live])) == live.sum()
    view = np.asarray([(5 * b + 2) % V for b in range(B)], np.int32)
    table = np.zeros((B, V, IMG), np.float32)
    table[vp[live]] = X_img[live]
    return vp, view, table, live


@pytest.mark.parametrize('case', AC.VISUAL_INDEX, ids=lambda c: 'V%d-IMG%d-LOC%d' % (c.V, c.IMG, c.LOC))
def test_visual_index_form_fp32_and_fp16(sf, case):
    """Index form (table row || location row) at small and full IMG / LOC, one sample at vp = -1 (all-zero panorama: zero
    output, uniform weights); a table of binary16-representable values gives the same bits from fp16 and fp32 storage,
    forward and backward."""
    c = case
    B, V, IMG, LOC, F = c.B, c.V, c.IMG, c.LOC, c.IMG + c.LOC
    loc = AC.loc_table(V, LOC)
    s = AC.visual_selection(B, V, F, hot=IMG, bits=11)
    vp, view, table, live = index_inputs(B, V, IMG, LOC, s.X[:, :, :IMG])
    Xs = AC.dense_panorama(table, loc, vp, view)
    assert AC.selection_is_one_hot(Xs[live], s.q[live], s.sel[live])
    rng = np.random.default_rng([V, IMG, LOC])
    Xd_img = AC.visual_dense(B, V, IMG)[0].astype(np.float16).astype(np.float32)
    _, _, table_d, _ = index_inputs(B, V, IMG, LOC, Xd_img)
    Xd = AC.dense_panorama(table_d, loc, vp, view)
    _, wd = AC.visual_dense(B, V, F)
    dout = rng.standard_normal((B, F)).astype(np.float32)
    vp_d, view_d = dev(vp), dev(view)
    got = {}
    for dtype, kernel, kbwd in (('fp32', c.kernel, AC.VIS_BWD), ('fp16', AC.half_name(c.kernel), AC.half_name(AC.VIS_BWD))):
        what = 'V%d IMG%d LOC%d %s' % (V, IMG, LOC, dtype)
        store = sf.features.FeatureStore(table, loc=LOC, dtype=dtype)
        assert_exact(host(store.loc_table), loc, what + ' loc table')
        rows, out, alpha, t_v, q = run_visual_fwd(sf, store.pano(vp_d, view_d), B, V, F, AC.visual_selection_weights(s))
        assert_ran(rows, kernel, what)
        assert_exact(q, s.q, what + ' q')
        ref_a = one_hot(B, V, s.sel)
        assert_exact(alpha[:B][live], ref_a[live], what + ' alpha')
        assert_exact(out[:B, :F][live], Xs[np.arange(B), s.sel][live], what + ' out')
        assert not out[:B, :F][~live].any() and np.abs(alpha[:B][~live] - 1.0 / V).max() <= 1e-7, what + ' vp = -1'
        assert AC.outside_is_untouched(out, B, F) and AC.outside_is_untouched(alpha, B, V)
        store_d = sf.features.FeatureStore(table_d, loc=LOC, dtype=dtype)
        pano_d = store_d.pano(vp_d, view_d)
        rows, out, alpha, t_v, q = run_visual_fwd(sf, pano_d, B, V, F, wd)
        check_dense_forward(Xd, rows, out, alpha, q, kernel, what + ' dense')
        a32 = np.ascontiguousarray(alpha[:B])
        rows, dq, dh, cols = run_visual_bwd(sf, pano_d, B, V, F, a32, dout)
        assert_ran(rows, kbwd, what + ' backward')
        check_e(dq, AC.visual_bwd(Xd, a32, dout), AC.visual_bwd(Xd, a32, dout, np.float32), what + ' dq')
        assert not dq[~live].any()
        got[dtype] = (out, alpha, dq, dh)
    for a, b, name in zip(got['fp32'], got['fp16'], ('out', 'alpha', 'dq', 'dh')):
        assert_exact(b, a, 'fp16 vs fp32 storage: ' + name)


@pytest.mark.parametrize('case', AC.VISUAL_BWD, ids=lambda c: 'V%d-F%d' % (c.V, c.F))
def test_visual_backward(sf, case):
    """sf_visual_attention_bwd, lddo = F + 4 with NaN padding: the exact family (dyadic alpha, small integers) bit for bit
    in dq and in dh = dq[:, cols]; the dense family within the bound."""
    c = case
    B, V, F = c.B, c.V, c.F
    what = 'backward V%d F%d' % (V, F)
    x = AC.visual_bwd_exact(B, V, F)
    pano, keep = dense_pano(sf, x.X)
    rows, dq, dh, cols = run_visual_bwd(sf, pano, B, V, F, x.alpha, x.dout)
    assert_ran(rows, c.kernel, what)
    assert_exact(dq, x.dq, what + ' exact dq')
    assert_exact(dh, x.dq[:, cols], what + ' exact dh')
    X, w = AC.visual_dense(B, V, F)
    alpha = AC.visual_fwd(X, AC.visual_query(w)[1], np.float32)[0]
    dout = (np.random.default_rng([V, F]).standard_normal((B, F)) * (1.0 + np.arange(F) % 3)[None, :]).astype(np.float32)
    pano, keep = dense_pano(sf, X)
    rows, dq, dh, cols = run_visual_bwd(sf, pano, B, V, F, alpha, dout)
    assert_ran(rows, c.kernel, what)
    check_e(dq, AC.visual_bwd(X, alpha, dout), AC.visual_bwd(X, alpha, dout, np.float32), what + ' dq')
    assert_exact(dh, dq[:, cols], what + ' dh is a copy of columns of dq')


@pytest.mark.parametrize('case', AC.VISUAL_F64, ids=lambda c: 'V%d-F%d' % (c.V, c.F))
def test_visual_forward_float64_scores(sf, case):
    """sf_visual_attention_fwd_f64 where visual_attn_f64_supported holds: the selection family exact, the dense family
    to the bound of tests/test_gpu_precise.py against the float64 evaluation from the float64 query."""
    c = case
    s = AC.visual_selection(c.V, c.V, c.F)
    pano, keep = dense_pano(sf, s.X)
    rows, out, alpha, t_v, q = run_visual_fwd(sf, pano, c.V, c.V, c.F, AC.visual_selection_weights(s),
                                              entry='sf_visual_attention_fwd_f64')
    check_selection_forward(s, rows, out, alpha, q, c.kernel, 'f64 V%d F%d selection' % (c.V, c.F))
    X, w = AC.visual_dense(c.B, c.V, c.F)
    pano, keep = dense_pano(sf, X)
    rows, out, alpha, t_v, q = run_visual_fwd(sf, pano, c.B, c.V, c.F, w, entry='sf_visual_attention_fwd_f64')
    assert_ran(rows, c.kernel, 'f64 dense')
    a64, o64 = AC.visual_fwd(X, AC.visual_query(w, f64)[1])
    ea, eo = float(np.abs(alpha[:c.B] - a64).max()), float(np.abs(out[:c.B, :c.F] - o64).max())
    print('[f64 scores V%d F%d] |dalpha| = %.2e, |dout| = %.2e at max|out| %.2f' % (c.V, c.F, ea, eo, np.abs(o64).max()))
    assert ea <= 1e-6 and eo <= 5e-6 * max(1.0, float(np.abs(o64).max()))
    assert AC.outside_is_untouched(out, c.B, c.F) and AC.outside_is_untouched(alpha, c.B, c.V)


@pytest.mark.parametrize('shift', [-60.0, 60.0])
@pytest.mark.parametrize('V', [AC.V_SPLIT_LO + 1, AC.V_MAX])
def test_split_merge_with_one_group_far_below_the_other(sf, V, shift):
    """The scores of views 0 .. 17 (the first workgroup's) about 60 below / above those of the second: the merge rescales
    one group's partials by e^-60, nothing underflows, the result stays within the dense family's bound."""
    B, F = 3, 260
    X, w = AC.visual_dense(B, V, F)
    X = AC.shift_scores(X, AC.visual_query(w)[1], slice(0, AC.VSP_RPG), shift)
    pano, keep = dense_pano(sf, X)
    rows, out, alpha, t_v, q = run_visual_fwd(sf, pano, B, V, F, w)
    sc = np.einsum('bvf,bf->bv', X.astype(f64), q.astype(f64))
    gap = sc[:, AC.VSP_RPG:].mean(1) - sc[:, :AC.VSP_RPG].mean(1)
    assert (np.abs(gap + shift) < 15.0).all(), gap
    check_dense_forward(X, rows, out, alpha, q, AC.VIS_SPLIT, 'merge V%d shift %+.0f' % (V, shift))


@pytest.mark.parametrize('F', [260, 2176])
@pytest.mark.parametrize('V', [AC.V_SPLIT_LO, AC.V_MAX], ids=['unsplit', 'split'])
def test_visual_train_mode_is_eval_times_the_oracle_mask(sf, V, F):
    """sf_dropout p = 0.5 with a non-zero drop_col0: out = (eval out) x the mask of oracle/rng.py, exactly (the scale is
    2); backward: the mask applied to dout in the kernel = the same call on dout x mask."""
    B, seed, row0, site, col0 = 3, 1234, 17, 9, 40
    X, w = AC.visual_dense(B, V, F)
    pano, keep = dense_pano(sf, X)
    kernel = AC.visual_fwd_kernel(V, B)
    rows, out0, alpha0, _, _ = run_visual_fwd(sf, pano, B, V, F, w)
    rows, out1, alpha1, _, _ = run_visual_fwd(sf, pano, B, V, F, w, drop=sf.dropout_arg(0.5, seed, row0), stream=site, col0=col0)
    assert_ran(rows, kernel, 'train mode')
    mask = orng.dropout_mask(seed, site, np.arange(row0, row0 + B), col0 + F, 0.5)[:, col0:]
    assert 0.3 < float((mask == 0).mean()) < 0.7
    assert_exact(out1[:B, :F], out0[:B, :F] * mask, 'train-mode out')
    assert_exact(alpha1, alpha0, 'train-mode alpha')
    assert AC.outside_is_untouched(out1, B, F)
    dout = np.random.default_rng(F).standard_normal((B, F)).astype(np.float32)
    a = np.ascontiguousarray(alpha0[:B])
    rows, dq1, dh1, _ = run_visual_bwd(sf, pano, B, V, F, a, dout, drop=sf.dropout_arg(0.5, seed, row0), stream=site, col0=col0)
    assert_ran(rows, AC.VIS_BWD, 'train-mode backward')
    rows, dq0, dh0, _ = run_visual_bwd(sf, pano, B, V, F, a, dout * mask)
    assert_exact(dq1, dq0, 'train-mode dq')
    assert_exact(dh1, dh0, 'train-mode dh')


# ================================================================================================== text attention
def txt_id(c):
    return 'L%d-H%d' % (c.L, c.H)


def run_text_fwd(sf, ctx, mask, t, ldt, ldwc):
    B, L, H = ctx.shape
    cd, td, md = dev(AC.layout(ctx.reshape(B * L, H))), dev(AC.layout(t, ldt)), dev(mask)
    alpha, wc = sentinel(B, L), sentinel(B, H, ldwc)
    with sf.profile() as prof:
        sf.call('sf_text_attention_fwd', sf.ptr(cd), sf.ptr(md), B, L, H, sf.ptr(td), ldt, sf.ptr(alpha), sf.ptr(wc), ldwc,
                sf.stream())
    torch.cuda.synchronize()
    return prof.rows, host(alpha), host(wc)


def run_text_bwd(sf, ctx, t, alpha, dwc, dctx0, lds):
    """lds = (lddwc, ldt, lddt).  -> (rows, dt buffer, dctx buffer [B L + 2, H] or None)."""
    B, L, H = ctx.shape
    lddwc, ldt, lddt = lds
    cd, td, ad, dd = dev(AC.layout(ctx.reshape(B * L, H))), dev(AC.layout(t, ldt)), dev(alpha), dev(AC.layout(dwc, lddwc))
    dt = sentinel(B, H, lddt)
    dctx = None if dctx0 is None else dev(AC.layout(dctx0.reshape(B * L, H), fill=SENT))
    with sf.profile() as prof:
        sf.call('sf_text_attention_bwd', sf.ptr(cd), B, L, H, sf.ptr(dd), lddwc, sf.ptr(td), ldt, sf.ptr(ad), sf.ptr(dt), lddt,
                sf.ptr(dctx), sf.stream())
    torch.cuda.synchronize()
    return prof.rows, host(dt), (None if dctx is None else host(dctx))


@pytest.mark.parametrize('case', AC.TEXT, ids=txt_id)
def test_text_forward(sf, case):
    """sf_text_attention_fwd: the selection family with B = L (every position designated once; without a mask and with
    the designated position's neighbour masked), the dense family at B = 3 under the three masks; ldt / ldwc contiguous and
    `H + 4 j`, j in {1, 3}, poisoned; alpha followed by a sentinel."""
    c = case
    L, H, what = c.L, c.H, txt_id(c)
    s = AC.text_selection(L, L, H)
    for (jt, jw), mask in (((0, 0), None), ((1, 3), AC.neighbour_mask(L)), ((3, 1), None)):
        rows, alpha, wc = run_text_fwd(sf, s.X, mask, s.q, H + 4 * jt, H + 4 * jw)
        assert_ran(rows, c.kernel, what)
        assert_exact(alpha[:L], np.eye(L, dtype=np.float32), what + ' selection alpha')
        assert_exact(wc[:L, :H], s.X[np.arange(L), s.sel], what + ' selection wc')
        assert AC.outside_is_untouched(wc, L, H) and AC.outside_is_untouched(alpha, L, L), what + ': wrote outside'
    B = c.B
    ctx, t, _, _ = AC.text_dense(B, L, H)
    for (jt, jw), kind in zip(((3, 1), (0, 0), (1, 3)), AC.MASKS):
        mask = AC.text_mask(kind, B, L)
        rows, alpha, wc = run_text_fwd(sf, ctx, mask, t, H + 4 * jt, H + 4 * jw)
        assert_ran(rows, c.kernel, what)
        a64, w64 = AC.text_fwd(ctx, t, mask)
        a32, w32 = AC.text_fwd(ctx, t, mask, np.float32)
        check_e(alpha[:B], a64, a32, '%s %s alpha' % (what, kind))
        check_e(wc[:B, :H], w64, w32, '%s %s wc' % (what, kind))
        if mask is not None:
            assert not alpha[:B][mask.astype(bool)].any(), what + ': weight on a masked position'
        assert AC.outside_is_untouched(wc, B, H) and AC.outside_is_untouched(alpha, B, L), what + ': wrote outside'


@pytest.mark.parametrize('case', AC.TEXT, ids=txt_id)
def test_text_backward(sf, case):
    """sf_text_attention_bwd: dt, and dctx accumulated onto a non-zero dctx, within the bound under the three masks (the
    mask reaches the backward as zeros of alpha); lddwc / ldt / lddt padded and poisoned; without dctx the same dt bits."""
    c = case
    B, L, H, what = c.B, c.L, c.H, txt_id(c)
    ctx, t, dwc, dctx0 = AC.text_dense(B, L, H)
    for lds, kind in zip(((H, H, H), (H + 4, H + 12, H + 4), (H + 12, H + 4, H + 12)), AC.MASKS):
        alpha = AC.text_fwd(ctx, t, AC.text_mask(kind, B, L), np.float32)[0]
        rows, dt, dctx = run_text_bwd(sf, ctx, t, alpha, dwc, dctx0, lds)
        assert_ran(rows, c.kernel, what)
        r64, r32 = AC.text_bwd(ctx, t, alpha, dwc, dctx0), AC.text_bwd(ctx, t, alpha, dwc, dctx0, np.float32)
        check_e(dt[:B, :H], r64[0], r32[0], '%s %s dt' % (what, kind))
        check_e(dctx[:B * L].reshape(B, L, H), r64[1], r32[1], '%s %s dctx' % (what, kind))
        assert AC.outside_is_untouched(dt, B, H) and AC.outside_is_untouched(dctx, B * L, H), what + ': wrote outside'
        rows, dt2, _ = run_text_bwd(sf, ctx, t, alpha, dwc, None, lds)
        assert_ran(rows, c.kernel, what)
        assert_exact(dt2, dt, what + ' dt without dctx')


def softdot_w(sf, w_in, w_out):
    tw = [dev(w_in), dev(w_out)]
    tw += [tw[0].t().contiguous(), tw[1].t().contiguous()]
    return sf.L.SoftdotW(*(t.data_ptr() for t in tw)), tw


@pytest.mark.parametrize('L,H', [(17, 260), (80, 512)])
def test_soft_dot_attention_ctx_row_equals_the_gathered_context(sf, L, H):
    """sf_soft_dot_attention_fwd with ctx_row: 7 rows over 3 contexts, repeated and out of order, bit for bit the run on
    the gathered dense context; the module's outputs against np_model at TOL; the module's backward against autograd."""
    rng = np.random.default_rng([L, H])
    n, B = 3, 7
    ctx_row = np.asarray([2, 0, 1, 1, 2, 0, 2], np.int32)
    ctx3, _, _, _ = AC.text_dense(n, L, H)
    mask3 = AC.text_mask('ragged', n, L)
    w_in = (rng.standard_normal((H, H)) * 0.5 * H ** -0.5).astype(np.float32)
    w_out = (rng.standard_normal((H, 2 * H)) * (2 * H) ** -0.5).astype(np.float32)
    h = (rng.standard_normal((B, H)) * 0.5).astype(np.float32)
    sw, keep = softdot_w(sf, w_in, w_out)
    hd = dev(h)

    def run(ctx, mask, row):
        cd, md, rd = dev(ctx), dev(mask), dev(row)
        outs = [torch.empty(B, H, device='cuda'), torch.empty(B, L, device='cuda'), torch.empty(B, 2 * H, device='cuda'),
                torch.empty(B, H, device='cuda')]
        with sf.profile() as prof:
            sf.call('sf_soft_dot_attention_fwd', C.byref(sw), B, L, H, sf.ptr(hd), H, sf.ptr(cd), sf.ptr(md), sf.ptr(rd),
                    *(sf.ptr(o) for o in outs), *sf.ws_args(hd.device))
        torch.cuda.synchronize()
        assert_ran(prof.rows, AC.text_kernel(L), 'soft dot L%d' % L)
        return outs
    via_row = run(ctx3, mask3, ctx_row)
    gathered = run(ctx3[ctx_row], mask3[ctx_row], None)
    for a, b, name in zip(via_row, gathered, ('h_tilde', 'alpha', 'cat2', 't_text')):
        assert torch.equal(a, b), name + ': ctx_row differs from the gathered context'
    ctx, mask = ctx3[ctx_row], mask3[ctx_row].astype(bool)
    ref_ht, ref_alpha = np_model.soft_dot_attention(h, ctx, mask, w_in, w_out)
    np.testing.assert_allclose(host(via_row[0]), ref_ht, **TOL)
    np.testing.assert_allclose(host(via_row[1]), ref_alpha, **TOL)
    # the module's backward on the gathered context
    go = rng.standard_normal((B, H)).astype(np.float32)
    th, tc = torch.tensor(h, requires_grad=True), torch.tensor(ctx, requires_grad=True)
    tht, _ = torch_ref.soft_dot_attention(th, tc, torch.tensor(mask), torch.tensor(w_in), torch.tensor(w_out))
    (tht * torch.tensor(go)).sum().backward()
    dh, dctx, cd, god = torch.empty(B, H, device='cuda'), torch.zeros(B, L, H, device='cuda'), dev(ctx), dev(go)
    ht, alpha, cat2, t_text = gathered
    with sf.profile() as prof:
        sf.call('sf_soft_dot_attention_bwd', C.byref(sw), None, B, L, H, sf.ptr(cd), sf.ptr(alpha), sf.ptr(cat2),
                sf.ptr(t_text), sf.ptr(ht), sf.ptr(god), sf.ptr(dh), H, sf.ptr(dctx), *sf.ws_args(hd.device))
    torch.cuda.synchronize()
    assert_ran(prof.rows, AC.text_kernel(L), 'soft dot backward L%d' % L)
    np.testing.assert_allclose(host(dh), th.grad.numpy(), **TOL)
    np.testing.assert_allclose(host(dctx), tc.grad.numpy(), **TOL)


# ========================================================================================================= scoring
def scoring_w(sf, w):
    tw = [dev(a) for a in w]
    tw += [tw[2].t().contiguous(), tw[0].t().contiguous()]
    return sf.L.ScoringW(*(t.data_ptr() for t in tw)), tw


def dense_cands(sf, U):
    """A dense sf_cands over U [B, A, F], two NaN rows behind the last row of the last sample."""
    Ud = dev(AC.layout(U.reshape(-1, U.shape[2])))
    return sf.L.Cands(Ud.data_ptr(), None, None, None, None, None, U.shape[1], 1, U.shape[2], 0), Ud


def run_score_fwd(sf, cands, B, A, F, h, w):
    H, D = h.shape[1], w[0].shape[0]
    sw, keep = scoring_w(sf, w)
    hd, logit = dev(h), sentinel(B, A)
    t_a, wt, r = torch.empty(B, D, device='cuda'), torch.empty(B, D, device='cuda'), torch.empty(B, F, device='cuda')
    with sf.profile() as prof:
        sf.call('sf_eltwise_prod_scoring_fwd', C.byref(sw), C.byref(cands), B, H, D, sf.ptr(hd), sf.ptr(logit), sf.ptr(t_a),
                sf.ptr(wt), sf.ptr(r), *sf.ws_args(hd.device))
    torch.cuda.synchronize()
    return prof.rows, host(logit), host(wt), host(r)


def run_score_bwd(sf, cands, B, A, F, dlogit):
    """sf_eltwise_prod_scoring_bwd with wt = identity rows: dr = rows < B of the W_a gradient, dc = the b_a gradient.
    -> (rows, dr, dc, dh, weights)."""
    D = AC.round4(max(B, 8))
    rng = np.random.default_rng([B, A, F, 5])
    w = ((rng.standard_normal((D, D)) * 0.3).astype(np.float32), np.zeros(D, np.float32),
         (rng.standard_normal((D, F)) * F ** -0.5).astype(np.float32), (rng.standard_normal(D) * 0.1).astype(np.float32),
         (rng.standard_normal((1, D)) * 0.5).astype(np.float32), np.zeros(1, np.float32))
    sw, keep = scoring_w(sf, w)
    wt = np.zeros((B, D), np.float32)
    wt[np.arange(B), np.arange(B)] = 1.0
    gwa, gba = torch.zeros(D, F, device='cuda'), torch.zeros(D, device='cuda')
    sg = sf.L.ScoringW(None, None, gwa.data_ptr(), gba.data_ptr(), None, None, None, None)
    hd, wtd, dl, dh = dev(np.zeros((B, D), np.float32)), dev(wt), dev(AC.layout(dlogit)), torch.empty(B, D, device='cuda')
    with sf.profile() as prof:
        sf.call('sf_eltwise_prod_scoring_bwd', C.byref(sw), C.byref(sg), C.byref(cands), B, D, D, sf.ptr(hd), sf.ptr(wtd),
                sf.ptr(wtd), sf.ptr(dl), sf.ptr(dh), *sf.ws_args(hd.device))
    torch.cuda.synchronize()
    gw, gb = host(gwa), host(gba)
    assert not gw[B:].any() and not gb[B:].any()
    return prof.rows, gw[:B], gb[:B], host(dh), w


def check_score_backward(sf, cands, U, kernel, what):
    """The exact family (one-hot 2^e dlogit: dr is a scaled copy of one candidate row) and the dense family."""
    B, A, F = U.shape
    rng = np.random.default_rng([B, A, F, 6])
    sel, val = np.arange(B) % A, (rng.choice([-1.0, 1.0], B) * 2.0 ** rng.integers(-3, 4, B)).astype(np.float32)
    dlogit = np.zeros((B, A), np.float32)
    dlogit[np.arange(B), sel] = val
    rows, dr, dc, _, _ = run_score_bwd(sf, cands, B, A, F, dlogit)
    assert_ran(rows, kernel, what)
    assert_exact(dr, U[np.arange(B), sel] * val[:, None], what + ' exact dr')
    assert_exact(dc, val, what + ' exact dc')
    dlogit = (rng.standard_normal((B, A)) * (1.0 + np.arange(A) % 3)[None, :]).astype(np.float32)
    rows, dr, dc, dh, w = run_score_bwd(sf, cands, B, A, F, dlogit)
    assert_ran(rows, kernel, what)
    r64, r32 = AC.score_bwd(U, dlogit), AC.score_bwd(U, dlogit, np.float32)
    check_e(dr, r64[0], r32[0], what + ' dr')
    check_e(dc, r64[1], r32[1], what + ' dc')

    def dh_of(drc, dt):          # dh = ((dr W_a^T + dc b_a) * w_out) W_h, the products behind the kernel
        w_h, _, w_a, b_a, w_out, _ = (a.astype(dt) for a in w)
        return ((drc[0].astype(dt) @ w_a.T + drc[1].astype(dt)[:, None] * b_a[None, :]) * w_out[0][None, :]) @ w_h
    check_e(dh, dh_of(r64, f64), dh_of(r32, np.float32), what + ' dh')
    return dr, dc, dh


def check_score_dense_forward(U, rows, logit, wt, r, w, kernel, what):
    B, A, F = U.shape
    assert_ran(rows, kernel, what)
    c64, c32 = AC.score_const(wt, w[3], w[5][0]), AC.score_const(wt, w[3], w[5][0], np.float32)
    check_e(logit[:B], AC.score_fwd(U, r, c64), AC.score_fwd(U, r, c32, np.float32), what + ' logit')
    assert AC.outside_is_untouched(logit, B, A), what + ': wrote behind logit'


@pytest.mark.parametrize('case', AC.SCORE, ids=lambda c: 'A%d-F%d' % (c.A, c.F))
def test_scoring_dense_source(sf, case):
    """sf_eltwise_prod_scoring_fwd / _bwd on dense candidates: every logit of the selection family exact, the dense
    family within the bound and against np_model at TOL; the backward's dr / dc exact and, with dh, within the bound."""
    c = case
    B, A, F, what = c.B, c.A, c.F, 'score A%d F%d' % (c.A, c.F)
    s = AC.score_selection(8, A, F)
    cands, keep = dense_cands(sf, s.U)
    rows, logit, wt, r = run_score_fwd(sf, cands, 8, A, F, s.h, s.w)
    assert_ran(rows, c.kernel, what)
    assert_exact(r, s.r, what + ' r (the 0 / 2^e weights must copy)')
    assert_exact(logit[:8], AC.score_selection_logits(s.U, s.r, s.cst, s.f0), what + ' selection logit')
    assert AC.outside_is_untouched(logit, 8, A)
    U, h, w = AC.score_dense(B, A, F)
    cands, keep = dense_cands(sf, U)
    rows, logit, wt, r = run_score_fwd(sf, cands, B, A, F, h, w)
    check_score_dense_forward(U, rows, logit, wt, r, w, c.kernel, what)
    np.testing.assert_allclose(logit[:B], np_model.eltwise_prod_scoring(h, U, *w), **TOL)
    check_score_backward(sf, cands, U, AC.SCORE_BWD, what + ' backward')


@pytest.mark.parametrize('case', AC.SCORE_INDEX, ids=lambda c: 'A%d-IMG%d-LOC%d' % (c.A, c.IMG, c.LOC))
def test_scoring_index_form_fp32_and_fp16(sf, case):
    """Index form: a_num in {1, A} and ragged, one row at vp = -1; the stop row, rows >= a_num and the vp = -1 sample give
    exactly the row constant; fp16 storage of binary16-representable values gives the fp32 bits, forward and backward."""
    c = case
    B, A, IMG, LOC, F, V = c.B, c.A, c.IMG, c.LOC, c.IMG + c.LOC, 6
    rng = np.random.default_rng([A, IMG, LOC])
    table = AC.full_mantissa(rng, B, V, IMG, bits=11)
    table_d = AC.visual_dense(B, V, IMG)[0].astype(np.float16).astype(np.float32)
    vp = np.asarray([3, 0, 4, -1, 1][:B], np.int32)
    a_num = np.asarray([1, A, max(1, A // 2), A, min(A, 3)][:B], np.int32)
    cand_view = rng.integers(0, V, (B, A)).astype(np.int32)
    ang = rng.uniform(-3.0, 3.0, (B, A, 2))
    sincos = sf.features.cand_sincos(ang[..., 0], ang[..., 1] * 0.3)
    idx = [dev(vp), dev(cand_view), dev(sincos), dev(a_num)]
    Us = AC.dense_candidates(table, vp, cand_view, sincos, a_num, LOC)
    Ud = AC.dense_candidates(table_d, vp, cand_view, sincos, a_num, LOC)
    dead = ~Us.any(2)
    assert dead[:, 0].all() and dead[3].all() and (A == 1 or not dead[1, 1:].any())
    s = AC.score_selection(B, A, F, U=Us)
    _, hd_, wd = AC.score_dense(B, A, F)
    got = {}
    for dtype, kf, kb in (('fp32', c.kernel, AC.SCORE_BWD), ('fp16', AC.half_name(c.kernel), AC.half_name(AC.SCORE_BWD))):
        what = 'score A%d IMG%d LOC%d %s' % (A, IMG, LOC, dtype)
        store = sf.features.FeatureStore(table, loc=LOC, dtype=dtype)
        rows, logit, wt, r = run_score_fwd(sf, store.cands(*idx, A), B, A, F, s.h, s.w)
        assert_ran(rows, kf, what)
        assert_exact(r, s.r, what + ' r')
        want = AC.score_selection_logits(Us, s.r, s.cst, s.f0)
        assert_exact(logit[:B], want, what + ' selection logit')
        assert_exact(logit[:B][dead], np.broadcast_to(s.cst[:, None], (B, A))[dead], what + ' stop / padding rows')
        store_d = sf.features.FeatureStore(table_d, loc=LOC, dtype=dtype)
        cands_d = store_d.cands(*idx, A)
        rows, logit, wt, r = run_score_fwd(sf, cands_d, B, A, F, hd_, wd)
        check_score_dense_forward(Ud, rows, logit, wt, r, wd, kf, what + ' dense')
        got[dtype] = (logit,) + check_score_backward(sf, cands_d, Ud, kb, what + ' backward')
    for a, b, name in zip(got['fp32'], got['fp16'], ('logit', 'dr', 'dc', 'dh')):
        assert_exact(b, a, 'fp16 vs fp32 storage: ' + name)


# ======================================================================================================= refusals
def refused(sf, status, what, fn):
    with sf.profile() as prof:
        with pytest.raises(sf.L.SfError, match=r'\(status %d\)' % status):
            fn()
    torch.cuda.synchronize()
    assert attention_kernels(prof.rows) == [], '%s: launched %s' % (what, sorted(prof.rows))


@pytest.mark.parametrize('case', AC.REFUSALS, ids=lambda r: r.entry + '-' + r.what.replace(' ', ''))
def test_one_step_past_each_limit_is_refused(sf, case):
    """Argument checking only: valid, finite inputs of a shape one step past a limit.  The call raises with
    SF_ERR_UNSUPPORTED, no attention kernel is launched, out / alpha / logit (backward: dh / dt) keep their sentinel."""
    d, B = case.dims, 3
    if case.entry == 'visual':
        V, F, ldo = d['V'], d['F'], d.get('ldo', AC.round4(d['F']))
        X, w = AC.visual_dense(B, V, F)
        pano, keep = dense_pano(sf, X)
        vw, keepw = visual_w(sf, w)
        h, out, alpha = dev(w.h), sentinel(B, F, ldo), sentinel(B, V)
        t_v, q = torch.empty(B, 32, device='cuda'), torch.empty(B, AC.round4(F), device='cuda')
        for entry in ('sf_visual_attention_fwd', 'sf_visual_attention_fwd_f64'):
            refused(sf, case.status, case.what, lambda: sf.call(
                entry, C.byref(vw), C.byref(pano), B, 32, 32, sf.ptr(h), sf.ptr(out), ldo, sf.ptr(alpha), sf.ptr(t_v),
                sf.ptr(q), None, 0, 0, *sf.ws_args(h.device)))
        assert AC.outside_is_untouched(host(out), 0, 0) and AC.outside_is_untouched(host(alpha), 0, 0)
        a0, tv0, do, dh = dev(np.full((B, V), 1.0 / V, np.float32)), dev(np.zeros((B, 32), np.float32)), dev(X[:, 0, :]), sentinel(B, 32)
        refused(sf, case.status, case.what + ' backward', lambda: sf.call(
            'sf_visual_attention_bwd', C.byref(vw), None, C.byref(pano), B, 32, 32, sf.ptr(h), sf.ptr(a0), sf.ptr(tv0),
            sf.ptr(do), d.get('ldo', F), None, 0, 0, sf.ptr(dh), *sf.ws_args(h.device)))
        assert AC.outside_is_untouched(host(dh), 0, 0)
    elif case.entry == 'text':
        L, H = d['L'], d['H']
        ctx, t, dwc, _ = AC.text_dense(B, L, H)
        cd, td, dd = dev(ctx), dev(t), dev(dwc)
        alpha, wc = sentinel(B, L), sentinel(B, H)
        refused(sf, case.status, case.what, lambda: sf.call(
            'sf_text_attention_fwd', sf.ptr(cd), None, B, L, H, sf.ptr(td), H, sf.ptr(alpha), sf.ptr(wc), H, sf.stream()))
        a0 = dev(np.full((B, L), 1.0 / L, np.float32))
        refused(sf, case.status, case.what, lambda: sf.call(
            'sf_text_attention_bwd', sf.ptr(cd), B, L, H, sf.ptr(dd), H, sf.ptr(td), H, sf.ptr(a0), sf.ptr(wc), H, None,
            sf.stream()))
        assert AC.outside_is_untouched(host(wc), 0, 0) and AC.outside_is_untouched(host(alpha), 0, 0)
    else:
        A, F = d['A'], d['F']
        U, h, w = AC.score_dense(B, A, F)
        cands, keep = dense_cands(sf, U)
        sw, keepw = scoring_w(sf, w)
        hd, logit = dev(h), sentinel(B, A)
        t_a, wt, r = torch.empty(B, 32, device='cuda'), torch.empty(B, 32, device='cuda'), torch.empty(B, F, device='cuda')
        refused(sf, case.status, case.what, lambda: sf.call(
            'sf_eltwise_prod_scoring_fwd', C.byref(sw), C.byref(cands), B, 32, 32, sf.ptr(hd), sf.ptr(logit), sf.ptr(t_a),
            sf.ptr(wt), sf.ptr(r), *sf.ws_args(hd.device)))
        assert AC.outside_is_untouched(host(logit), 0, 0)
        z, dl, dh = dev(np.zeros((B, 32), np.float32)), dev(np.ones((B, A), np.float32)), sentinel(B, 32)
        refused(sf, case.status, case.what + ' backward', lambda: sf.call(
            'sf_eltwise_prod_scoring_bwd', C.byref(sw), None, C.byref(cands), B, 32, 32, sf.ptr(hd), sf.ptr(z), sf.ptr(z),
            sf.ptr(dl), sf.ptr(dh), *sf.ws_args(hd.device)))
        assert AC.outside_is_untouched(host(dh), 0, 0)


def test_fp16_flag_with_a_dense_source(sf):
    """Planned as a refusal (SF_ERR_ARG); the ABI never tags a dense source as half, so a sf_pano / sf_cands naming a
    registered binary16 table beside a dense tensor runs the fp32 dense kernel on the dense rows -- the same bits as
    without the table pointer (the table, of the dense tensor's full size, holds other values)."""
    B, V, A, F = 3, 19, 4, 64
    store = sf.features.FeatureStore(np.ones((B, V, F), np.float32), loc=4, dtype='fp16')
    assert sf.L.lib.sf_feature_table_is_f16(C.c_void_p(store.table.data_ptr())) == 1
    X, w = AC.visual_dense(B, V, F)
    pano, keep = dense_pano(sf, X)
    plain = run_visual_fwd(sf, pano, B, V, F, w)
    tagged = sf.L.Pano(keep.data_ptr(), store.table.data_ptr(), None, None, None, V, F, 0)
    rows, out, alpha, t_v, q = run_visual_fwd(sf, tagged, B, V, F, w)
    assert_ran(rows, AC.VIS_SPLIT, 'dense source beside an fp16 table')
    assert_exact(out, plain[1], 'out')
    assert_exact(alpha, plain[2], 'alpha')
    U, h, ws_ = AC.score_dense(B, A, F)
    cands, keepu = dense_cands(sf, U)
    plain = run_score_fwd(sf, cands, B, A, F, h, ws_)
    tagged = sf.L.Cands(keepu.data_ptr(), store.table.data_ptr(), None, None, None, None, A, 1, F, 0)
    rows, logit, wt, r = run_score_fwd(sf, tagged, B, A, F, h, ws_)
    assert_ran(rows, AC.SCORE_FWD, 'dense candidates beside an fp16 table')
    assert_exact(logit, plain[1], 'logit')


# ================================================================================== the deferred context gradient
@pytest.mark.parametrize('case', AC.CTX_GRAD, ids=lambda c: 'L%d-S%d' % (c.L, c.S))
def test_deferred_context_gradient_on_both_sides_of_its_limits(sf, case):
    """Follower teacher-forced training passes built as in tests/test_gpu_grads_f64.py (B = 3, full-size models, float64
    oracle, tests/grad_compare.py): the longest instruction fills L = 80 / 81 positions; at L = 80 the episode has 102 / 103
    steps (S L = 8160 / 8240 around the 8192 that fit ctx_grad_kernel's LDS).  ctx_grad_kernel runs exactly where
    ctx_grad_supported holds; the context gradient (every encoder gradient behind it) matches the oracle either way."""
    from tests.test_gpu_grads_f64 import _follower, _check_case
    c = case
    assert AC.ctx_grad_supported(c.S, c.L, AC.H_MAX) == c.runs

    def longest(fb):
        fb.instr[0] = np.random.default_rng(c.L).integers(4, synth.FULL.vocab, c.L - 1).astype(np.int64)     # + EOS = L positions
    r = _follower(3, c.S, train=True, seed=61 + c.L, min_len=5, max_len=40, stop_prob=0.0, mutate=longest, max_length=c.L)
    assert r['st'].ctx.shape[1] == c.L
    _check_case('ctx grad L=%d S=%d' % (c.L, c.S), r)
    with sf.profile() as prof:
        r['run']()
    assert (AC.CTX_GRAD_KERNEL in prof.rows) == c.runs, sorted(prof.rows)
    assert any(k.startswith('text_attn_kernel') for k in prof.rows)
