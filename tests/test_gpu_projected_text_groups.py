"""GPU: launch (1) of the projected decode chain with TWO text groups per sample (csrc/sf_attention.hip:
text_fold_body<RPW, 2> inside pair_proj_textfold_kernel<RPW, true, 2>) against the four-group form of the same build and
against the float64 numpy oracle.

Two groups hold 8 * RPW positions each, RPW from the ladder 1, 2, 3, 5 at ceil(L / 16): so L runs over both sides of
every rung (8 | 9: the second group appears, 16 | 17, 32 | 33, 48 | 49: rung 5 stands in for 4, 64 | 65, 80) and L = 81,
where the two-group ladder ends and a forced 2 must not run two.  (The engine folds the text attention up to 80 positions
only -- follower.py -- so at L = 81 no launch (1) runs at all and both settings issue the same unfolded steps; the
launcher's own limit, the same `L <= 80` term that gates the rule, is held by tests/test_projected_text_groups_host.py.)
Every batch holds rows whose second group is all
padding (it only draws its tickets), a row with exactly ONE live position in the second group, and a row of length 1.

The per-sample tickets are never reset and are shared by every launch on a workspace: a two-group block adds 2, a
four-group block 1, so both forms, the unprojected chain and a captured graph are run in turn on one engine and must
each repeat their first result bit for bit.

Bounds: those of tests/test_gpu_projected.py -- against the oracle actions equal and logits within 1e-4; two groups
against four, actions equal and logits within 3e-5 x the logit scale (the same fp32 sums in another order).
Every test sets the switch itself and restores the default; none depends on test order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from oracle import np_env, np_model                                   # noqa: E402
from tests.follower_models import full_size_models                    # noqa: E402

NVP = 32
_cache = {}


def _models(seed=77):
    if seed not in _cache:
        _cache[seed] = full_size_models(seed)
    return _cache[seed]


class groups:
    """`with groups(n):` -- the process-wide switch (0: the rule), restored to the rule on exit."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from speaker_follower_amd import _lib
        _lib.lib.sf_debug_projected_text_groups(self.n)

    def __exit__(self, *exc):
        from speaker_follower_amd import _lib
        _lib.lib.sf_debug_projected_text_groups(0)


def _lengths(B, L):
    """Row lengths (EOS included), longest first: L itself; around the end of the first of two groups (LG = 8 * RPW):
    LG + 1 (one live position in the second group), LG and LG - 1 (second group all padding); a row of length 1 last."""
    rpw = -(-L // 16)
    lg = 8 * (rpw if rpw <= 3 else 5)
    rng = np.random.default_rng(1000 + L)
    want = [L, lg + 1, lg, lg - 1, lg // 2, 1]
    lens = [n for n in want if 1 <= n <= L]
    lens += [int(n) for n in rng.integers(1, L + 1, size=B - len(lens))]
    lens = sorted(lens, reverse=True)
    assert lens[0] == L and lens[-1] == 1 and len(lens) == B
    if L > lg:
        assert lg + 1 in lens
    return lens


def _batch(B, S, lens, seed):
    fb = synth.follower_batch(seed=seed, batch=B, steps=S, n_viewpoints=NVP, min_len=2, max_len=12)
    rng = np.random.default_rng(seed + 7)
    fb.instr = [rng.integers(4, synth.FULL.vocab, size=n - 1).astype(np.int64) for n in lens]   # (+ EOS = n)
    return fb


def _rollout(eng, batch, S):
    from speaker_follower_amd import _lib
    with torch.no_grad():
        with _lib.kernel_profile() as prof:
            st = eng.rollout(batch, S, 'argmax', train=False)
            torch.cuda.synchronize()
    return st, sorted(prof.rows)


def _launch1(names):
    """The group counts of the launches (1) that carried the partials, from their profile names."""
    out = set()
    for k in names:
        if 'pair_proj_textfold_kernel' in k and 'true' in k:
            out.add(int(k.rsplit(',', 1)[1].strip(' >)')))
    return out


@pytest.mark.parametrize('L', [1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81])
def test_two_groups_match_four_groups_and_the_oracle(L):
    from speaker_follower_amd import features, follower
    enc, dec, enc_w, dec_w = _models()
    B, S, MAXLEN = 16, 3, 96
    lens = _lengths(B, L)
    fb = _batch(B, S, lens, seed=300 + L)
    table = synth.feature_table(5, NVP)
    store = features.FeatureStore(table)
    batch = follower.DeviceFollowerBatch.from_synth(fb, max_length=MAXLEN)
    assert batch.mask.shape[1] == L and batch.lengths == lens
    seq, mask, rlens = np_env.batch_instructions_from_encoded(fb.instr, MAXLEN, reverse=True)
    loc = np_env.static_loc_embeddings()
    ref = np_model.follower_rollout(enc_w, dec_w, seq, rlens, mask, S,
                                    lambda t: np_env.dense_follower_step(table, loc, fb, t), fb.target, 'argmax', 2176,
                                    early_exit=False)
    n = len(ref['logits'])
    got = {}
    for force in (2, 4):
        eng = follower.FollowerEngine(enc, dec, store)
        eng.project = True
        with groups(force):
            st, names = _rollout(eng, batch, S)
        assert bool(st.text_folded) == (L <= 80) and bool(st.projected) == (L <= 80)
        ran = _launch1(names)
        # (L = 81: never two, even when two is forced -- the engine does not fold there, so no launch (1) at all)
        assert ran == ({2} if force == 2 and L <= 80 else {4} if L <= 80 else set()), names
        lg, ac = st.logits.cpu().numpy().copy(), st.actions.cpu().numpy().copy()
        got[force] = (lg, ac)
        # against the float64 oracle
        assert np.array_equal(ac[:n], ref['actions'])
        worst = 0.0
        for t in range(n):
            a = ref['logits'][t].shape[1]
            ok = np.isfinite(ref['logits'][t])
            worst = max(worst, float(np.abs(lg[t][:, :a][ok] - ref['logits'][t][ok]).max()))
        print('[L=%d, %d groups ran as %s] max |logit - oracle| %.2e' % (L, force, sorted(ran), worst))
        assert worst <= 1e-4
    (l2, a2), (l4, a4) = got[2], got[4]
    fin = np.isfinite(l4)
    assert np.array_equal(fin, np.isfinite(l2))
    scale = float(np.abs(l4[fin]).max())
    d = float(np.abs(l2[fin] - l4[fin]).max())
    print('[L=%d] max |logit| %.2f, two groups vs four %.2e (3e-5 * scale = %.2e)' % (L, scale, d, 3e-5 * max(scale, 1.0)))
    assert d <= 3e-5 * max(scale, 1.0)
    assert np.array_equal(a2, a4)
    if L > 80:
        assert d == 0.0                                              # (the same launches under either setting)


def test_tickets_stay_aligned_across_forms_on_one_workspace():
    """One engine: forced 2, forced 4, the unprojected chain, forced 2 again, then a captured forced-2 graph replayed three
    times -- each equal, bit for bit, to the first result of its own kind."""
    from speaker_follower_amd import features, follower
    enc, dec, _, _ = _models()
    B, S, L = 16, 3, 33
    fb = _batch(B, S, _lengths(B, L), seed=41)
    store = features.FeatureStore(synth.feature_table(5, NVP))
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    eng = follower.FollowerEngine(enc, dec, store)

    def run(project, force):
        eng.project = project
        with groups(force):
            st, names = _rollout(eng, batch, S)
        assert bool(st.projected) == project
        if project:
            assert _launch1(names) == {force}, names
        return st.logits.clone(), st.actions.clone()

    first2 = run(True, 2)
    first4 = run(True, 4)
    plain = run(False, 0)
    again2 = run(True, 2)
    again4 = run(True, 4)
    plain2 = run(False, 0)
    for a, b in ((first2, again2), (first4, again4), (plain, plain2)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(first2[1], first4[1]) and torch.equal(first2[1], plain[1])
    eng.project = True
    with groups(2):
        replay, gst = eng.capture(batch, S, 'argmax')
    assert gst.projected
    run(True, 4)                                        # (the workspace's tickets move on between capture and replay)
    for _ in range(3):
        replay()
        torch.cuda.synchronize()
        assert torch.equal(gst.logits, first2[0]) and torch.equal(gst.actions, first2[1])
    after = run(True, 2)
    assert torch.equal(after[0], first2[0])


def test_the_rule_picks_two_groups_at_batch_100_and_four_at_16():
    """The switch at 0: B = 100 with L = 80 is the first shape whose four-group grid (732 blocks) does not fit the device at
    once and reports two groups; B = 16 (144 blocks) reports four.  The rule's choice at B = 100 -- 532 blocks, more than
    one wave of workgroups per CU -- also agrees with a forced four."""
    from speaker_follower_amd import features, follower
    enc, dec, _, _ = _models()
    S = 2
    store = features.FeatureStore(synth.feature_table(5, NVP))
    out = {}
    for B, want in ((100, 2), (16, 4)):
        fb = synth.follower_batch(seed=90 + B, batch=B, steps=S, n_viewpoints=NVP, min_len=1, max_len=79)
        fb.instr[0] = np.arange(4, 4 + 79, dtype=np.int64)          # 79 tokens + EOS: L = 80
        batch = follower.DeviceFollowerBatch.from_synth(fb)
        assert batch.mask.shape[1] == 80
        for force in (0, 4):
            eng = follower.FollowerEngine(enc, dec, store)
            eng.project = True
            with groups(force):
                st, names = _rollout(eng, batch, S)
            assert st.projected
            assert _launch1(names) == {want if force == 0 else 4}, names
            out[B, force] = (st.logits.cpu().numpy().copy(), st.actions.cpu().numpy().copy())
    (lr, ar), (l4, a4) = out[100, 0], out[100, 4]
    fin = np.isfinite(l4)
    scale = max(float(np.abs(l4[fin]).max()), 1.0)
    assert np.array_equal(fin, np.isfinite(lr)) and np.array_equal(ar, a4)
    assert float(np.abs(lr[fin] - l4[fin]).max()) <= 3e-5 * scale
    assert np.array_equal(out[16, 0][0], out[16, 4][0])              # (the same launches: the same bits)
