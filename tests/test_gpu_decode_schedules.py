"""GPU: WHICH kernels each schedule of the follower's decode step launches (csrc/sf_api_follower.hip: decoder_tail_i picks one of
five launch chains per step -- the projected chain, the four-launch folded chain, the paired unfolded one, its query-only
variant for a device-resident environment, the plain step).

The numeric tests cannot see a wrong choice: a folded rollout that silently falls back to another chain still passes
tests/test_gpu_text_fold.py.  Here one eager rollout per case runs under the library's own launch profile
(_lib.kernel_profile) and its {kernel name: calls} table is compared with decode_schedules.json next to this file.

The table is a recording of the schedules as they were BEFORE the decode step was split into one function per chain:

    python tests/test_gpu_decode_schedules.py --record tests/decode_schedules.json

run at that commit with this module copied into it -- never a recording of the code under test.  Re-record only with a
change that is meant to alter a schedule, and say so."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

from speaker_follower_amd import synth                                # noqa: E402
from tests.follower_models import full_size_models                    # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'decode_schedules.json')

# case -> engine switches, rollout arguments and shape (defaults: B = 16, S = 3, 32 viewpoints, instruction lengths
# 2..12, no_grad, 'argmax', train=False).  'paired257' is not a schedule of its own: it is what 'fallback' must equal.
CASES = {
    'folded4': dict(),
    'paired': dict(engine=dict(fold_text=False)),
    'train': dict(feedback='teacher', train=True, grad=True),             # (dropout on; forward only)
    'per-call': dict(engine=dict(fold_text=False, episode_call=False)),
    'plain': dict(engine=dict(pipelined=False)),
    'nav folded': dict(nav=True),
    'nav unfolded': dict(nav=True, engine=dict(fold_text=False)),
    'fallback': dict(B=257, S=2),                                          # (above VIS_SPLIT_MAX_B: no folded chain)
    'paired257': dict(B=257, S=2, engine=dict(fold_text=False)),
}

_world = {}


def _nav_world():
    if not _world:
        import search_world as W
        from speaker_follower_amd import features, nav
        env, table = W.build_world(dense=False, n_items=24, batch=12)
        store = features.FeatureStore(table)
        env.reset_epoch()
        env._next_minibatch(True)
        _world.update(store=store, table=nav.NavTable(env, store), items=list(env.batch))
    return _world


def run_case(name):
    """One warm-up rollout, then one eager rollout under the launch profile: ({kernel name: calls}, its state)."""
    from speaker_follower_amd import _lib, features, follower, nav
    case = CASES[name]
    B, S = case.get('B', 16), case.get('S', 3)
    enc, dec, _, _ = full_size_models()
    if case.get('nav'):
        w = _nav_world()
        store = w['store']
        make_batch = lambda: nav.DeviceNavBatch(w['table'], w['items'], S)          # noqa: E731  (it holds the walk's state)
    else:
        fb = synth.follower_batch(seed=11 + B, batch=B, steps=S, n_viewpoints=32, min_len=2, max_len=12)
        store = features.FeatureStore(synth.feature_table(5, 32))
        batch = follower.DeviceFollowerBatch.from_synth(fb)
        make_batch = lambda: batch                                                   # noqa: E731
    eng = follower.FollowerEngine(enc, dec, store)
    for k, v in case.get('engine', {}).items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    with torch.set_grad_enabled(bool(case.get('grad'))):
        eng.rollout(make_batch(), S, case.get('feedback', 'argmax'), train=bool(case.get('train')))
        torch.cuda.synchronize()
        with _lib.kernel_profile() as prof:
            st = eng.rollout(make_batch(), S, case.get('feedback', 'argmax'), train=bool(case.get('train')))
            torch.cuda.synchronize()
    return {k: v['calls'] for k, v in sorted(prof.rows.items())}, st


@pytest.fixture(scope='module')
def recorded():
    with open(TABLE) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def seen():
    """{case: {kernel name: calls}} of the cases run so far (each runs once, whichever test asks first)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_case(name)[0]
        return cache[name]
    return get


@pytest.mark.parametrize('name', list(CASES))
def test_schedule_launches_the_recorded_kernels(name, seen, recorded):
    got = seen(name)
    print('[%s] %d kernels, %d launches' % (name, len(got), sum(got.values())))
    for k in sorted(set(got) | set(recorded[name])):
        if got.get(k) != recorded[name].get(k):
            print('    %-90s now %s, recorded %s' % (k, got.get(k), recorded[name].get(k)))
    assert got == recorded[name]


def test_the_two_chains_are_two_different_schedules(seen):
    assert seen('folded4') != seen('paired')


def test_above_the_split_limit_the_step_is_the_paired_one(seen):
    """B = 257 is above VIS_SPLIT_MAX_B: the folded chains decline before their first launch and every step is the
    paired unfolded one -- launch for launch the rollout with fold_text off at that shape, none of the folded kernels.
    The only launches on top are the two many-row products that build ctx_q / ctx_o: the episode issues them once, in
    front of step 0, before any step can decline."""
    fb, pd = seen('fallback'), seen('paired257')
    assert not [k for k in fb if 'pair_textfold' in k]
    extra = {k: fb[k] - pd.get(k, 0) for k in fb if fb[k] != pd.get(k, 0)}
    assert set(pd) <= set(fb) and extra == {'gemm_nt_big_kernel': 2}, extra


def test_the_per_call_loop_issues_the_paired_schedule(seen):
    assert seen('per-call') == seen('paired')


if __name__ == '__main__':
    out = sys.argv[sys.argv.index('--record') + 1]
    table = {}
    for case_name in CASES:
        table[case_name] = run_case(case_name)[0]
        print('%-14s %3d kernels, %4d launches' % (case_name, len(table[case_name]), sum(table[case_name].values())), flush=True)
    with open(out, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
