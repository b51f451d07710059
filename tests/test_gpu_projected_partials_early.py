"""GPU: the attention partials of the projected decode chain in launch (1) -- the early placement, the default -- at the
smallest shapes where their body (csrc/sf_attention.hip: proj_partials_body, merged by proj_merge_body) can go wrong.

The body splits a sample into three groups of twelve views; six waves hold two rows each, two waves form the scores from
the projected rows; a lane's nine row slots are typed image / location per slot.  So:
  * V = 19 (the lowest the chain takes: group 1 holds 7 views, group 2 none), V = 25 (group 2 holds exactly one view),
    V = 35 (odd: the last row wave holds a single live row) and V = 36;
  * (IMG, LOC) = (2048, 128): 512 + 32 chunks, the ninth slot half live; (48, 16): 12 + 4 chunks, seven slots never
    emitted;
  * H = 512 and H = 36 (nine chunks of a projected row: less than one 64-lane column);
  * B = 1 and B = 3, the latter with a padded sample (vp < 0: zero panorama, every score 0, alpha uniform).

Two routes, each case against a float64 numpy oracle AND against the late placement (launch (2): visual_split_body) of
the same build:
  * the engine, S = 2 decode steps -- exactly one paired step (launch (1) with the partials, launch (2) with their merge)
    and one last step -- at the full model dimensions, where the chain engages, with V below 36 from a narrower table;
  * sf_debug_projected_attention, the same two kernels with empty text and scoring parts on caller buffers, for the
    shapes no engine is built for (small rows, small H, a padded sample).

Bounds: those of tests/test_gpu_projected.py -- logits within 3e-5 x the logit scale (here also: the attended row within
3e-5 x its scale), actions equal, alpha_v rows summing to 1 within 1e-5 and matching within rtol 1e-4 / atol 1e-6.
Every test sets the placement switch itself and restores the default; none depends on test order."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from oracle import np_env, np_model                                   # noqa: E402
from tests.follower_models import full_size_models                    # noqa: E402

DEFAULT_LATE = 0            # the library's default placement (csrc/sf_api.hip: sf_debug_projected_partials_late)
NVP = 6
_cache = {}


def _models(seed=77):
    if seed not in _cache:
        _cache[seed] = full_size_models(seed)
    return _cache[seed]


class placement:
    """`with placement(late):` -- the process-wide switch, restored to the default on exit."""

    def __init__(self, late):
        self.late = late

    def __enter__(self):
        from speaker_follower_amd import _lib
        _lib.lib.sf_debug_projected_partials_late(self.late)

    def __exit__(self, *exc):
        from speaker_follower_amd import _lib
        _lib.lib.sf_debug_projected_partials_late(DEFAULT_LATE)


def _ran_early(names):
    return any('pair_proj_textfold_kernel' in k and 'true' in k for k in names)


# ================================================================================================ through the engine
def _rollout(eng, batch, S):
    from speaker_follower_amd import _lib
    with torch.no_grad():
        with _lib.kernel_profile() as prof:
            st = eng.rollout(batch, S, 'argmax', train=False)
            torch.cuda.synchronize()
    return st, set(prof.rows), (st.logits.cpu().numpy().copy(), st.actions.cpu().numpy().copy(),
                                st.tape['alpha_v'].cpu().numpy().copy())


@pytest.mark.parametrize('B,V', [(1, 19), (3, 25), (3, 35), (1, 36), (3, 36)])
def test_engine_early_placement_matches_the_oracle_and_the_late_placement(B, V):
    from speaker_follower_amd import features, follower
    enc, dec, enc_w, dec_w = _models()
    S = 2
    dims = dataclasses.replace(synth.FULL, views=V)
    fb = synth.follower_batch(seed=40 + V + B, batch=B, steps=S, n_viewpoints=NVP, min_len=2, max_len=12, dims=dims)
    fb.view[0, 0], fb.view[1, 0] = V - 1, 0                         # (the edges of the location table)
    fb.vp[1, B - 1] = NVP - 1
    table = synth.feature_table(5, NVP, dims)
    store = features.FeatureStore(table)
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    got = {}
    for name, project, late in (('folded', False, DEFAULT_LATE), ('early', True, 0), ('late', True, 1)):
        eng = follower.FollowerEngine(enc, dec, store)
        eng.project = project
        with placement(late):
            st, names, got[name] = _rollout(eng, batch, S)
        assert st.text_folded and bool(st.projected) == project
        if project:
            assert _ran_early(names) == (late == 0), sorted(names)
    lu, au, avu = got['folded']
    fin = np.isfinite(lu)
    scale = max(float(np.abs(lu[fin]).max()), 1.0)
    for name, other in (('early', 'folded'), ('late', 'folded'), ('early', 'late')):
        (la, aa, ava), (lb, ab, avb) = got[name], got[other]
        assert np.array_equal(np.isfinite(la), np.isfinite(lb))
        d = float(np.abs(la[fin] - lb[fin]).max())
        print('[B=%d V=%d] %s vs %s: max |logit| %.2f, logits %.2e, alpha_v %.2e' % (B, V, name, other, scale, d,
                                                                                   np.abs(ava - avb).max()))
        assert d <= 3e-5 * scale
        assert np.array_equal(aa, ab)
        np.testing.assert_allclose(ava.sum(-1), 1.0, atol=1e-5)
        np.testing.assert_allclose(ava, avb, rtol=1e-4, atol=1e-6)
    # the reference itself (numpy oracle)
    lp, ap, avp = got['early']
    seq, mask, lens = np_env.batch_instructions_from_encoded(fb.instr, 80, reverse=True)
    loc = np_env.static_loc_embeddings(V)
    ref = np_model.follower_rollout(enc_w, dec_w, seq, lens, mask, S,
                                    lambda t: np_env.dense_follower_step(table, loc, fb, t), fb.target, 'argmax', 2176,
                                    early_exit=False)
    n = len(ref['logits'])
    assert np.array_equal(ap[:n], ref['actions'])
    for t in range(n):
        a = ref['logits'][t].shape[1]
        ok = np.isfinite(ref['logits'][t])
        assert float(np.abs(lp[t][:, :a][ok] - ref['logits'][t][ok]).max()) <= 1e-4


# ================================================================================================ the two kernels alone
CASES = [  # B, V, IMG, LOC, H
    (1, 19, 2048, 128, 512),
    (3, 19, 48, 16, 36),
    (3, 25, 2048, 128, 36),
    (3, 25, 48, 16, 512),
    (3, 35, 2048, 128, 512),
    (1, 36, 48, 16, 36),
    (3, 36, 2048, 128, 512),
]
_refs = {}


def _case(B, V, IMG, LOC, H):
    """Inputs and the float64 oracle of one case, computed once: score_v = (PV[vp V + v] + LV[view V + v]) . [h1 | 1],
    alpha = softmax(score), out = sum_v alpha_v [table[vp, v] | loc[view, v]]; a padded sample (vp < 0) has a zero
    panorama and scores 0 everywhere."""
    key = (B, V, IMG, LOC, H)
    if key in _refs:
        return _refs[key]
    from tests import attention_cases as AC
    rng = np.random.default_rng([V, IMG, H, B])
    ld = (H + 1 + 3) // 4 * 4
    table = np.maximum(0.5 * rng.standard_normal((NVP, V, IMG)), 0.0).astype(np.float32)
    loc = AC.loc_table(V, LOC)
    sigma = 2.0 / np.sqrt(H)                                         # (scores spread over a few units: peaky weights)
    pv = np.zeros((NVP * V, ld), np.float32)
    lv = np.zeros((V * V, ld), np.float32)
    pv[:, :H + 1] = sigma * rng.standard_normal((NVP * V, H + 1))
    lv[:, :H + 1] = sigma * rng.standard_normal((V * V, H + 1))
    h1 = rng.uniform(-1.0, 1.0, (B, H)).astype(np.float32)
    vp = rng.integers(0, NVP, B).astype(np.int32)
    view = rng.integers(0, V, B).astype(np.int32)
    vp[0], view[0] = NVP - 1, V - 1                                 # (the last rows of every table)
    if B > 1:
        vp[1] = -1
    alpha = np.zeros((B, V))
    out = np.zeros((B, IMG + LOC))
    for b in range(B):
        if vp[b] < 0:
            alpha[b] = 1.0 / V
            continue
        rows = pv[vp[b] * V:(vp[b] + 1) * V].astype(np.float64) + lv[view[b] * V:(view[b] + 1) * V].astype(np.float64)
        s = rows[:, :H] @ h1[b].astype(np.float64) + rows[:, H]
        e = np.exp(s - s.max())
        alpha[b] = e / e.sum()
        x = np.concatenate((table[vp[b]], loc[view[b]]), axis=1).astype(np.float64)
        out[b] = alpha[b] @ x
    _refs[key] = dict(table=table, loc=loc, pv=pv, lv=lv, ld=ld, h1=h1, vp=vp, view=view, alpha=alpha, out=out)
    return _refs[key]


def _attention_alone(store, c, B, V, F, H, late):
    from speaker_follower_amd import _lib, runtime
    dev = store.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    pv, lv, h1, vp, view = t(c['pv']), t(c['lv']), t(c['h1']), t(c['vp']), t(c['view'])
    ldo = F + 4
    alpha = torch.full((B + 1, V), np.nan, device=dev)               # (a row behind the last sample: must stay untouched)
    out = torch.full((B + 1, ldo), np.nan, device=dev)
    pano = store.pano(vp, view)
    with _lib.kernel_profile() as prof:
        _lib.call('sf_debug_projected_attention', C.byref(pano), B, H, runtime.ptr(pv), runtime.ptr(lv), c['ld'],
                  runtime.ptr(h1), H, runtime.ptr(alpha), runtime.ptr(out), ldo, late, *runtime.ws_args(dev))
        torch.cuda.synchronize()
    assert _ran_early(set(prof.rows)) == (late == 0), sorted(prof.rows)
    alpha, out = alpha.cpu().numpy(), out.cpu().numpy()
    assert np.isnan(alpha[B]).all() and np.isnan(out[B]).all() and np.isnan(out[:B, F:]).all(), 'wrote outside alpha / out'
    return alpha[:B].astype(np.float64), out[:B, :F].astype(np.float64)


@pytest.mark.parametrize('B,V,IMG,LOC,H', CASES)
def test_partials_and_merge_alone_match_the_oracle_and_the_late_placement(B, V, IMG, LOC, H):
    from speaker_follower_amd import features
    c = _case(B, V, IMG, LOC, H)
    F = IMG + LOC
    store = features.FeatureStore(c['table'], loc=LOC)
    assert np.array_equal(store.loc_table.cpu().numpy(), c['loc'])
    a_early, o_early = _attention_alone(store, c, B, V, F, H, 0)
    a_late, o_late = _attention_alone(store, c, B, V, F, H, 1)
    scale = max(float(np.abs(c['out']).max()), 1.0)
    for name, (a, o), (ar, orf) in (('early vs oracle', (a_early, o_early), (c['alpha'], c['out'])),
                                    ('late vs oracle', (a_late, o_late), (c['alpha'], c['out'])),
                                    ('early vs late', (a_early, o_early), (a_late, o_late))):
        print('[B=%d V=%d IMG=%d LOC=%d H=%d] %s: alpha %.2e (max alpha %.3f), out %.2e at scale %.2f'
              % (B, V, IMG, LOC, H, name, np.abs(a - ar).max(), ar.max(), np.abs(o - orf).max(), scale))
        np.testing.assert_allclose(a.sum(-1), 1.0, atol=1e-5)
        np.testing.assert_allclose(a, ar, rtol=1e-4, atol=1e-6)
        assert float(np.abs(o - orf).max()) <= 3e-5 * scale
    if B > 1:                                                        # the padded sample: uniform weights, a zero row
        assert np.abs(a_early[1] - 1.0 / V).max() <= 1e-7 and not o_early[1].any()
