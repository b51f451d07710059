"""GPU: `sample` feedback through the FUSED carriers of the glue -- score_glue_kernel, pair_score_merge and the projected
pair_proj_score_kernel compile the same follower_glue_row (csrc/sf_glue.h) as the stand-alone kernel that
tests/test_gpu_choice_kernels.py section 6 holds to the float64 mirror; here the same rule is applied to whole rollouts.

One rollout per schedule (the models and batches of tests/test_gpu_decode_schedules.py: full size, B = 16, S = 4, 32
viewpoints, instruction lengths 2..12; a nav world of 12 items for the two device-environment cases), feedback 'sample',
a fixed dropout_seed and batch.row0 = 300.  For each:

    which chain ran      asserted from the state and the launch profile, so a fallback cannot pass for what it replaced
    draw by draw         actions[t, b] = oracle.rng.follower_sample(the launch's own masked logits[t, b], the uniform of
                         (dropout_seed ^ 0x1B873593, site0 + t, 300 + b)); clear / unclear rule and the float32-weight
                         rule of choice_models.check_draws; clear share over the rollout >= 0.99
    step_scores          log p(action) by choice_models.check_values
    it samples           some step holds more than one distinct action; the rollout differs from the argmax rollout
    the feedback path    (pre-drawn observations) a teacher rollout at the same seed and sites whose targets are the
                         sampled actions reproduces the logits of every (t, b) up to and including the step at which
                         row b first stops, bit for bit: what step t + 1 was fed is the row of the SAMPLED action
    the walk             (device environment) row / view after every step are the nav table's successor of the sampled
                         action, and in some row not the arg max's

Measured on an MI355X (score: worst e / e32 over the four steps, bound max(4 e32, 1e-5) = 1.0e-05 everywhere):

    folded         2.41e-07 / 2.36e-07        per-call       2.17e-07 / 2.03e-07        nav folded     1.63e-07 / 1.28e-07
    projected      3.33e-07 / 1.44e-07        plain          2.17e-07 / 2.03e-07        nav unfolded   1.93e-07 / 1.79e-07
    paired         2.17e-07 / 2.03e-07        train          3.04e-07 / 2.48e-07

Clear share 1.0000 in every case: none of the 64 (nav: 48) draws of a rollout came within 1e-5 of a cdf boundary, and
every one took the mirror's action.  The teacher rollout on the sampled actions reproduced the logits bit for bit in all
six pre-drawn cases, train mode (dropout 0.5 at the same sites) included: no launch reorders its sums between the two
feedbacks.  The module takes 3 to 4 s, its slowest case (the first: the models are built) 0.5 s.
"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from tests import choice_models as CM                                 # noqa: E402
from tests.follower_models import full_size_models                    # noqa: E402

F32 = np.float32
B, S, ROW0, SEED = 16, 4, 300, 0x5EED1234
SAMPLE_XOR = 0x1B873593                  # follower.py: the sampling seed is dropout_seed ^ this

# schedule -> engine switches, rollout arguments, and what must be true of the state / launch profile afterwards
CASES = {
    'folded': dict(engine=dict(project=False),
                   ran=lambda st, k: st.episode and st.text_folded and not st.projected and has(k, 'pair_score_merge_kernel')),
    'projected': dict(engine=dict(project=True),
                      ran=lambda st, k: st.episode and st.projected and has(k, 'pair_proj_score_kernel')),
    'paired': dict(engine=dict(fold_text=False),
                   ran=lambda st, k: st.episode and not st.text_folded and has(k, 'pair_vis_small_kernel', 'score_glue_kernel')
                   and not has(k, 'pair_textfold')),
    'per-call': dict(engine=dict(fold_text=False, episode_call=False),
                     ran=lambda st, k: st.episode is None and has(k, 'pair_vis_small_kernel', 'score_glue_kernel')),
    'plain': dict(engine=dict(pipelined=False),
                  ran=lambda st, k: st.episode is None and has(k, 'score_glue_kernel') and not has(k, 'pair_')),
    'train': dict(train=True, grad=True,
                  ran=lambda st, k: st.episode and not st.text_folded and st.drop_dec[0] == 0.5 and has(k, 'score_glue_kernel')),
    'nav folded': dict(nav=True,
                       ran=lambda st, k: st.episode and st.text_folded and has(k, 'pair_textfold', 'score_glue_kernel')
                       and k['nav_step_kernel'] == 1),
    'nav unfolded': dict(nav=True, engine=dict(fold_text=False),
                         ran=lambda st, k: st.episode and not st.text_folded and has(k, 'text_attn_kernel', 'score_glue_kernel')
                         and not has(k, 'pair_textfold') and k['nav_step_kernel'] == 1),
}
SEEN = {}                                # case -> (worst e, its e32, clear share), for the module's report


def has(kernels, *prefixes):
    return all(any(name.startswith(p) for name in kernels) for p in prefixes)


_world = {}


def nav_world():
    if not _world:
        import search_world as W
        from speaker_follower_amd import features, nav
        env, table = W.build_world(dense=False, n_items=12, batch=12)
        store = features.FeatureStore(table)
        env.reset_epoch()
        env._next_minibatch(True)
        _world.update(store=store, table=nav.NavTable(env, store), items=list(env.batch))
    return _world


def rollouts(name):
    """The sampled rollout of one case under the launch profile, and an argmax / a teacher-on-the-samples rollout with
    the same switches, seed and sites -> dict."""
    from speaker_follower_amd import _lib, features, follower, nav
    case = CASES[name]
    enc, dec, _, _ = full_size_models()
    if case.get('nav'):
        w = nav_world()
        store = w['store']
        make_batch = lambda target=None: nav.DeviceNavBatch(w['table'], w['items'], S, row0=ROW0)    # noqa: E731
    else:
        fb = synth.follower_batch(seed=11 + B, batch=B, steps=S, n_viewpoints=32, min_len=2, max_len=12)
        store = features.FeatureStore(synth.feature_table(5, 32))
        batch = follower.DeviceFollowerBatch.from_synth(fb, row0=ROW0)
        make_batch = lambda target=None: batch if target is None else dataclasses.replace(batch, target=target)   # noqa: E731
    eng = follower.FollowerEngine(enc, dec, store)
    eng.dropout_seed = SEED
    for k, v in case.get('engine', {}).items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    train = bool(case.get('train'))

    def run(feedback, batch, profile=False):
        eng.site_next = 128                                           # every rollout at the same sites
        with torch.set_grad_enabled(bool(case.get('grad'))):
            if not profile:
                st = eng.rollout(batch, S, feedback, train=train)
                torch.cuda.synchronize()
                return st, None
            with _lib.kernel_profile() as prof:
                st = eng.rollout(batch, S, feedback, train=train)
                torch.cuda.synchronize()
            return st, {k: v['calls'] for k, v in prof.rows.items()}

    run('sample', make_batch())                                       # warm-up: allocations, caches, projected tables
    b_s = make_batch()
    st, kernels = run('sample', b_s, profile=True)
    out = dict(st=st, batch=b_s, kernels=kernels, eng=eng)
    out['argmax'] = run('argmax', make_batch())[0]
    if not case.get('nav'):
        out['teacher'] = run('teacher', make_batch(st.actions.clone()))[0]
    return out


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    for name, (e, e32, share, n_unclear) in SEEN.items():
        print('[follower sample] %-13s score e / e32 = %.2e / %.2e   clear share %.4f (%d unclear)' % (name, e, e32, share, n_unclear))


@pytest.mark.parametrize('name', list(CASES))
def test_sampled_rollout_draw_by_draw(name):
    from speaker_follower_amd import _lib
    assert _lib.ABI_VERSION >= 8
    r = rollouts(name)
    st, batch = r['st'], r['batch']
    assert CASES[name]['ran'](st, r['kernels']), (name, sorted(r['kernels']))
    assert st.site0 == 128 and st.site_rel == 128 and batch.row0 == ROW0 and st.feedback == 2
    n = batch.batch_size
    logits = st.logits.cpu().numpy()
    actions = st.actions.cpu().numpy()
    scores = st.step_scores.cpu().numpy()
    a_num = batch.a_num[:S].cpu().numpy()
    A = logits.shape[2]
    assert logits.shape == (S, n, A) and actions.shape == (S, n)
    valid = np.arange(A)[None, None, :] < a_num[:, :, None]
    assert np.array_equal(np.isneginf(logits), ~valid) and np.isfinite(logits[valid]).all()      # the MASKED logits
    seed = (SEED ^ SAMPLE_XOR) & 0xFFFFFFFF
    clear, worst = [], (0.0, 0.0)
    for t in range(S):
        ex = CM.draw_expectation(logits[t], valid[t], CM.follower_uniforms(seed, st.site0 + t, ROW0, n))
        CM.check_draws('%s step %d' % (name, t), actions[t], logits[t], valid[t], ex)
        clear.append(ex['clear'])
        for _, e, e32 in CM.check_sample_scores('%s step %d' % (name, t), scores[t], logits[t], actions[t], np.zeros(n)):
            worst = max(worst, (e, e32))
    clear = np.concatenate(clear)
    SEEN[name] = worst + (float(clear.mean()), int((~clear).sum()))
    assert clear.mean() >= 0.99, clear.mean()
    assert max(len(set(actions[t].tolist())) for t in range(S)) > 1
    greedy = r['argmax'].actions.cpu().numpy()
    assert not np.array_equal(actions, greedy)
    assert np.array_equal(greedy[0], CM.first_max(logits[0]))         # (step 0 sees the same logits: it is the arg max)

    if 'teacher' in r:
        again = r['teacher']
        assert again.site0 == st.site0 and again.feedback == 0
        relog = again.logits.cpu().numpy()
        stops = actions == 0
        first = np.where(stops.any(0), stops.argmax(0), S - 1)       # the step at which row b first stops
        upto = np.arange(S)[:, None] <= first[None, :]
        assert upto[1:].any() and (first < S - 1).any()
        same = (logits.view(np.int32) == relog.view(np.int32)).all(2)
        assert same[upto].all(), '%s: teacher-on-the-samples differs at (t, b) %s' % (name, np.argwhere(upto & ~same)[:4].tolist())
        assert np.array_equal(again.actions.cpu().numpy()[upto], actions[upto])
    else:
        host = batch.nav.host
        V = len(host['a_num']) // batch.nav.n_rows                     # poses per nav row
        rows, views = batch.row[:S + 1].cpu().numpy(), batch.view[:S + 1].cpu().numpy()
        want_r, want_v, greedy_r = rows[:S].copy(), views[:S].copy(), rows[:S].copy()
        for t in range(S):
            s0 = rows[t].astype(np.int64) * V + views[t]
            for acts, out_r, out_v in ((actions[t], want_r, want_v), (CM.first_max(logits[t]), greedy_r, None)):
                act = np.where(acts >= host['a_num'][s0], 0, acts)
                nr = host['next_row'][s0, act]
                move = (act != 0) & (nr != rows[t])
                out_r[t] = np.where(move, nr, rows[t])
                if out_v is not None:
                    out_v[t] = np.where(move, host['cand_view'][s0, act], views[t])
        assert np.array_equal(rows[1:], want_r) and np.array_equal(views[1:], want_v)
        assert (want_r != greedy_r).any() and (rows[1:] != rows[:-1]).any()
        assert np.array_equal(batch.vp[1:S + 1].cpu().numpy(), host['feat_row'][rows[1:]])
