"""GPU: WHICH kernels one training iteration of the follower launches (csrc/sf_api_follower.hip: sf_follower_episode_bwd
walks the steps on one stream or on two -- heads on a side stream, tails behind their events -- and declines the second
stream above VIS_SPLIT_MAX_B; follower.FollowerEngine._backward calls it once).  The backward counterpart of tests/test_gpu_decode_schedules.py.

The numeric tests cannot see a wrong choice: a backward that silently takes another path still gives the reference's
gradients.  Here one eager training iteration per case -- rollout(..., 'teacher', train=True) with a fixed dropout seed,
loss.backward(), a synchronize -- runs under the library's own launch profile (_lib.kernel_profile, which sees the
launches of every host thread, autograd's included) and its {kernel name: calls} table is compared with
backward_schedules.json next to this file.

The table is a recording of the schedules as they were BEFORE the experiment switches left the backward through time:

    python tests/test_gpu_backward_schedules.py --record tests/backward_schedules.json

run at that commit with this module copied into it -- never a recording of the code under test.  Re-record only with a
change that is meant to alter a schedule, and say so.

The two streams of the backward order each other by events only, so the profile is safe on both."""
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

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'backward_schedules.json')

# case -> engine switches and shape (defaults: B = 16, S = 3, 32 viewpoints, instruction lengths 2..12, 'teacher',
# train=True).  'one-stream257' is not a schedule of its own: it is what 'above-split' must equal.
CASES = {
    'one-stream': dict(engine=dict(two_stream_backward=False)),
    'two-stream': dict(),
    'above-split': dict(B=257, S=2),                                       # (above VIS_SPLIT_MAX_B: one stream)
    'one-stream257': dict(B=257, S=2, engine=dict(two_stream_backward=False)),
}


def run_case(name):
    """One warm-up iteration, then one eager training iteration under the launch profile: {kernel name: calls}."""
    from speaker_follower_amd import _lib, features, follower
    case = CASES[name]
    B, S = case.get('B', 16), case.get('S', 3)
    enc, dec, _, _ = full_size_models()
    fb = synth.follower_batch(seed=11 + B, batch=B, steps=S, n_viewpoints=32, min_len=2, max_len=12)
    store = features.FeatureStore(synth.feature_table(5, 32))
    batch = follower.DeviceFollowerBatch.from_synth(fb)
    eng = follower.FollowerEngine(enc, dec, store)
    eng.dropout_seed = 99
    for k, v in case.get('engine', {}).items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)

    def iteration():
        st = eng.rollout(batch, S, 'teacher', train=True)
        st.loss.backward()
        torch.cuda.synchronize()

    iteration()
    with _lib.kernel_profile() as prof:
        iteration()
    return {k: v['calls'] for k, v in sorted(prof.rows.items())}


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
            cache[name] = run_case(name)
        return cache[name]
    return get


@pytest.mark.parametrize('name', list(CASES))
def test_iteration_launches_the_recorded_kernels(name, seen, recorded):
    got = seen(name)
    print('[%s] %d kernels, %d launches' % (name, len(got), sum(got.values())))
    for k in sorted(set(got) | set(recorded[name])):
        if got.get(k) != recorded[name].get(k):
            print('    %-90s now %s, recorded %s' % (k, got.get(k), recorded[name].get(k)))
    assert got == recorded[name]


def test_above_the_split_limit_the_walk_is_the_one_stream_one(seen):
    """B = 257 is above VIS_SPLIT_MAX_B: the two-stream walk declines, and the default engine's iteration is launch for
    launch the one with two_stream_backward off at that shape."""
    assert seen('above-split') == seen('one-stream257')


if __name__ == '__main__':
    out = sys.argv[sys.argv.index('--record') + 1]
    table = {}
    for case_name in CASES:
        table[case_name] = run_case(case_name)
        print('%-14s %3d kernels, %4d launches' % (case_name, len(table[case_name]), sum(table[case_name].values())), flush=True)
    with open(out, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
