"""CPU checks of tests/attention_cases.py: the float64 references against the oracle (np_model forward, float64 autograd of
torch_ref backward), the exact families really exact under a float32 evaluation, and the case tables on both sides of
every boundary the constants define."""
import numpy as np
import pytest
import torch

from oracle import np_model, torch_ref
from tests import attention_cases as AC

f64 = np.float64


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, f64), requires_grad=grad)


# ------------------------------------------------------------------------------- references vs the oracle
@pytest.mark.parametrize('B,V,F', [(3, 5, 24), (2, 19, 36)])
def test_visual_references_agree_with_the_oracle(B, V, F):
    X, w = AC.visual_dense(B, V, F, H=8, D=12)
    _, q = AC.visual_query(w, f64)
    alpha, out = AC.visual_fwd(X, q)
    ref_out, ref_alpha = np_model.visual_soft_dot_attention(w.h, X, w.w_h, w.b_h, w.w_v, w.b_v)
    np.testing.assert_allclose(alpha, ref_alpha, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(out, ref_out, rtol=2e-5, atol=2e-6)
    # backward: with W_h = W_v = identity the module's h IS the kernel's q, and d out / d h the kernel's dq
    rng = np.random.default_rng(B + V)
    qv, dout = rng.standard_normal((B, F)) * 0.3, rng.standard_normal((B, F))
    th = t64(qv, True)
    eye = t64(np.eye(F))
    tout, talpha = torch_ref.visual_soft_dot_attention(th, t64(X), eye, t64(np.zeros(F)), eye, t64(np.zeros(F)))
    (tout * t64(dout)).sum().backward()
    a64, _ = AC.visual_fwd(X, qv)
    np.testing.assert_allclose(a64, talpha.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(AC.visual_bwd(X, a64, dout), th.grad.numpy(), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize('B,L,H,kind', [(3, 7, 16, 'ragged'), (2, 70, 8, 'hole'), (3, 1, 4, 'none')])
def test_text_references_agree_with_the_oracle(B, L, H, kind):
    ctx, t, dwc, dctx0 = AC.text_dense(B, L, H)
    mask = AC.text_mask(kind, B, L)
    mb = None if mask is None else mask.astype(bool)
    alpha, wc = AC.text_fwd(ctx, t, mask)
    ref_wc, ref_alpha = np_model.context_only_soft_dot_attention(t, ctx, mb, np.eye(H, dtype=np.float32))
    np.testing.assert_allclose(alpha, ref_alpha, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(wc, ref_wc, rtol=2e-5, atol=2e-6)
    if mask is not None:
        assert float(alpha[mb].sum()) == 0.0
    th, tc = t64(t, True), t64(ctx, True)
    twc, _ = torch_ref.context_only_soft_dot_attention(th, tc, None if mb is None else torch.tensor(mb), t64(np.eye(H)))
    (twc * t64(dwc)).sum().backward()
    dt, dctx, ds = AC.text_bwd(ctx, t, alpha, dwc, dctx0)
    np.testing.assert_allclose(dt, th.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dctx - dctx0, tc.grad.numpy(), rtol=1e-9, atol=1e-11)
    # ds is the gradient of the scores: dt = ds . ctx, and it sums to zero over the live positions
    np.testing.assert_allclose(ds.sum(1), 0.0, atol=1e-12)


@pytest.mark.parametrize('B,A,F', [(3, 4, 24), (1, 16, 12)])
def test_scoring_references_agree_with_the_oracle(B, A, F):
    U, h, w = AC.score_dense(B, A, F, H=8, D=12)
    w_h, b_h, w_a, b_a, w_out, b_out = w
    wt = (h.astype(f64) @ w_h.astype(f64).T + b_h) * w_out[0].astype(f64)
    r = wt @ w_a.astype(f64)
    logit = AC.score_fwd(U, r, AC.score_const(wt, b_a, b_out[0]))
    np.testing.assert_allclose(logit, np_model.eltwise_prod_scoring(h, U, *w), rtol=2e-5, atol=2e-6)
    # backward: W_h = W_a = identity, w_out = 1: the module's h is r, d logit / d h = dr + dc b_a, d / d b_out = sum dc
    rng = np.random.default_rng(A)
    dlogit, ba = rng.standard_normal((B, A)), rng.standard_normal(F)
    th, tb = t64(rng.standard_normal((B, F)), True), t64([0.25], True)
    eye = t64(np.eye(F))
    tl = torch_ref.eltwise_prod_scoring(th, t64(U), eye, t64(np.zeros(F)), eye, t64(ba), t64(np.ones((1, F))), tb)
    (tl * t64(dlogit)).sum().backward()
    dr, dc = AC.score_bwd(U, dlogit)
    np.testing.assert_allclose(dr + dc[:, None] * ba[None, :], th.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(dc.sum(), tb.grad.numpy()[0], rtol=1e-12)


# ------------------------------------------------------------------------------------- the exact families
@pytest.mark.parametrize('B,V,F,bits', [(36, 36, 2304, 24), (19, 19, 4, 24), (5, 2, 260, 11), (257, 36, 64, 24), (3, 1, 8, 24)])
def test_visual_selection_is_one_hot_and_exact_in_float32(B, V, F, bits):
    s = AC.visual_selection(B, V, F, bits=bits)
    assert AC.selection_is_one_hot(s.X, s.q, s.sel)
    alpha, out = AC.visual_fwd(s.X, s.q, np.float32)
    onehot = np.zeros((B, V), np.float32)
    onehot[np.arange(B), s.sel] = 1.0
    assert alpha.dtype == np.float32 and np.array_equal(alpha, onehot)
    assert np.array_equal(out, s.X[np.arange(B), s.sel])
    if B >= V:
        assert set(s.sel) == set(range(V))                           # every row designated once
    if bits == 11:
        assert np.array_equal(s.X.astype(np.float16).astype(np.float32), s.X)
    # the 0 / 2^e weights reproduce q exactly, as (at most) two exact products per element
    w = AC.visual_selection_weights(s)
    t_v, q = AC.visual_query(w, f64)
    assert np.array_equal(q, s.q.astype(f64)) and np.array_equal(AC.visual_query(w, np.float32)[1], s.q)
    for m in (w.h, w.w_h, w.w_v):
        nz = np.abs(m[m != 0]).astype(f64)
        assert np.array_equal(np.log2(nz), np.rint(np.log2(nz)))     # 0 / 2^e only
    assert ((w.w_h != 0).sum(1) == 1).all()
    assert float(((t_v != 0).astype(f64) @ (w.w_v != 0).astype(f64)).max()) <= 2.0      # non-zero products per element


@pytest.mark.parametrize('L,H', [(128, 512), (17, 4), (1, 260), (81, 252)])
def test_text_selection_is_one_hot_and_exact_in_float32(L, H):
    s = AC.text_selection(L, L, H)
    for mask in (None, AC.neighbour_mask(L)):
        assert AC.selection_is_one_hot(s.X, s.q, s.sel, mask)
        alpha, wc = AC.text_fwd(s.X, s.q, mask, np.float32)
        assert np.array_equal(alpha, np.eye(L, dtype=np.float32)) and np.array_equal(wc, s.X[np.arange(L), s.sel])


@pytest.mark.parametrize('B,A,F', [(8, 16, 2304), (3, 1, 4), (5, 15, 260)])
def test_scoring_selection_gives_single_product_logits(B, A, F):
    s = AC.score_selection(B, A, F)
    w_h, b_h, w_a, b_a, w_out, b_out = s.w
    wt = (s.h.astype(f64) @ w_h.astype(f64).T + b_h) * w_out[0].astype(f64)
    assert np.array_equal(wt @ w_a.astype(f64), s.r.astype(f64))
    assert np.array_equal(AC.score_const(wt, b_a, b_out[0]), s.cst.astype(f64))
    assert ((s.r != 0).sum(1) == 1).all()
    want = AC.score_selection_logits(s.U, s.r, s.cst, s.f0)
    assert np.array_equal(AC.score_fwd(s.U, s.r, s.cst, np.float32), want)
    np.testing.assert_allclose(np_model.eltwise_prod_scoring(s.h, s.U, *s.w), want, rtol=1e-5, atol=1e-5)
    assert len(np.unique(want)) > B * A // 2


@pytest.mark.parametrize('B,V,F', [(3, 36, 2304), (3, 1, 4), (3, 19, 260)])
def test_visual_backward_exact_family_is_exact_in_float32(B, V, F):
    c = AC.visual_bwd_exact(B, V, F)
    assert np.array_equal(AC.visual_bwd(c.X, c.alpha, c.dout, np.float32), c.dq)
    assert float(np.abs(c.dq).max()) > 0.0
    t_v, w_h, w_v, cols = AC.copy_weights(B, F)
    assert np.array_equal(t_v.T.astype(f64) @ c.dq.astype(f64), np.vstack((c.dq, np.zeros((len(cols) - B, F)))))
    assert np.array_equal(c.dq.astype(f64) @ w_v.astype(f64).T @ w_h.astype(f64), c.dq[:, cols].astype(f64))


def test_dense_family_spreads_are_a_few_units():
    X, w = AC.visual_dense(3, 36, 2304)
    s = np.einsum('bvf,bf->bv', X.astype(f64), AC.visual_query(w, f64)[1])
    assert 1.0 < float(s.max() - s.min()) < 40.0
    ctx, t, _, _ = AC.text_dense(3, 128, 512)
    st = np.einsum('blh,bh->bl', ctx.astype(f64), t.astype(f64))
    assert 1.0 < float(st.max() - st.min()) < 40.0
    # the imbalanced merge: one group about 60 below the other, nothing underflows
    q = AC.visual_query(w, f64)[1]
    s2 = np.einsum('bvf,bf->bv', AC.shift_scores(X, q, slice(0, AC.VSP_RPG), -60.0).astype(f64), q)
    np.testing.assert_allclose(s2[:, :AC.VSP_RPG], s[:, :AC.VSP_RPG] - 60.0, atol=1e-3)
    assert np.exp(float(s2.min() - s2.max())) > 4.0 * np.finfo(np.float32).tiny, float(s2.max() - s2.min())


# ---------------------------------------------------------------------------------------- the case tables
def test_case_tables_hold_both_sides_of_every_boundary():
    for name, table, field, below, above in AC.boundaries():
        values = {getattr(c, field) for c in table}
        assert below in values, '%s: no case at %s = %d' % (name, field, below)
        if above is not None:
            assert above in values, '%s: no case at %s = %d' % (name, field, above)
        else:
            entry = name.split()[0]
            assert any(r.entry == entry and r.dims.get(field, -1) > below for r in AC.REFUSALS), name + ': no refusal'


def test_cases_name_the_kernel_the_dispatch_picks():
    for c in AC.VISUAL:
        assert c.kernel == AC.visual_fwd_kernel(c.V, c.B) and c.F % 4 == 0 and c.F <= AC.F_MAX and 1 <= c.V <= AC.V_MAX
    assert {c.kernel for c in AC.VISUAL if c.V <= AC.V_SPLIT_LO} == {AC.VIS_FWD}
    assert {c.kernel for c in AC.VISUAL if c.V > AC.V_SPLIT_LO and c.B <= AC.VIS_SPLIT_MAX_B} == {AC.VIS_SPLIT}
    assert [c.kernel for c in AC.VISUAL if c.B > AC.VIS_SPLIT_MAX_B] == [AC.VIS_FWD]
    for c in AC.VISUAL_INDEX:
        assert c.kernel == AC.visual_fwd_kernel(c.V, c.B) and c.IMG % 4 == 0 and c.LOC % 4 == 0
    assert {c.kernel for c in AC.VISUAL_INDEX} == {AC.VIS_FWD, AC.VIS_SPLIT}
    assert all(AC.visual_f64_supported(c.V, c.B, c.F) for c in AC.VISUAL_F64)
    for c in AC.TEXT:
        assert c.kernel == AC.text_kernel(c.L) and c.H % 4 == 0
    assert {c.kernel for c in AC.TEXT} == {AC.TXT % r for r in AC.TXT_RPW}
    assert {(c.L, c.H) for c in AC.TEXT} == {(L, H) for L in AC.TXT_L for H in AC.TXT_H}
    assert AC.text_kernel(AC.L_MAX + 1) is None
    for c in AC.SCORE_INDEX:
        assert c.LOC % AC.SCORE_LOC_MULTIPLE == 0 and c.IMG % 4 == 0
    assert AC.half_name(AC.VIS_FWD) == 'visual_attn_kernel<0, true>' and AC.half_name(AC.SCORE_FWD) == 'score_fwd_kernel<f16>'


def test_deferred_context_gradient_cases_straddle_its_limits():
    H = AC.H_MAX
    for c in AC.CTX_GRAD:
        assert AC.ctx_grad_supported(c.S, c.L, H) == c.runs
    L = (AC.CG_THREADS // (H // 4)) * AC.CG_ROWS
    assert {c.L for c in AC.CTX_GRAD} >= {L, L + 1}
    s_max = AC.CG_LDS // (8 * L)
    assert {c.S for c in AC.CTX_GRAD if c.L == L} == {s_max, s_max + 1}
