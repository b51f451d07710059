"""CPU: bench.py --dump-outputs -- what the files hold (float32 / float64, integers exact, masked logits as a finite
value plus the mask), the 64 MB ceiling with its seeded sample (the same elements in every run), and --steps as the
number of timed steps (at least one)."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    argv = sys.argv
    sys.argv = ['bench.py']
    try:
        spec = importlib.util.spec_from_file_location('sf_bench_dump_under_test', os.path.join(ROOT, 'bench.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def test_small_outputs_are_written_whole_as_float32_or_float64(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    arrays = dict(actions=rng.integers(0, 8, (20, 100)), logits=rng.standard_normal((20, 100, 8)).astype(np.float32),
                  ended=rng.integers(0, 2, 100).astype(bool), loss=np.array([1.25], np.float64),
                  half=rng.standard_normal(7).astype(np.float16))
    arrays['logits'][0, 0, 5:] = -np.inf                          # (written as given: step_outputs removes the mask)
    info = bench.dump_outputs(str(tmp_path / 'out'), arrays)
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(k + '.npy' for k in arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / 'out' / (name + '.npy'))
        assert got.dtype == (np.float32 if name in ('logits', 'half') else np.float64), name
        assert got.shape == a.shape and info[name] == (a.shape, False)
        np.testing.assert_array_equal(got, a.astype(got.dtype))


def test_a_large_set_is_sampled_under_the_ceiling_with_the_same_elements_every_time(tmp_path):
    bench = _bench()
    big = np.arange(2 * bench.DUMP_SAMPLE + 12345, dtype=np.float32) * 0.5
    arrays = dict(big=big, small=np.arange(10, dtype=np.int64))
    limit = big.nbytes // 2
    first = bench.dump_outputs(str(tmp_path / 'a'), arrays, limit=limit)
    second = bench.dump_outputs(str(tmp_path / 'b'), dict(arrays, big=big.copy()), limit=limit)
    assert first == second == dict(big=((bench.DUMP_SAMPLE,), True), small=((10,), False))
    a, b = (np.load(tmp_path / d / 'big.npy') for d in ('a', 'b'))
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, big))     # distinct elements in index order
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'small.npy'), np.arange(10.0))
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= limit


def test_the_default_ceiling_is_64_mb(tmp_path):
    bench = _bench()
    arrays = {'w%d' % i: np.ones(3_000_000, np.float32) for i in range(8)}        # 96 MB as given
    bench.dump_outputs(str(tmp_path), arrays)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6


def _state(rng, S, B, A, H):
    import torch
    a_num = torch.tensor(rng.integers(1, A + 1, (S, B)), dtype=torch.int32)
    logits = torch.tensor(rng.standard_normal((S, B, A)), dtype=torch.float32)
    logits[torch.arange(A) >= a_num[..., None]] = -float('inf')   # what the rollout's glue writes for a >= a_num
    return types.SimpleNamespace(batch=types.SimpleNamespace(a_num=a_num), logits=logits,
                                 actions=torch.tensor(rng.integers(0, A, (S, B))),
                                 step_scores=torch.tensor(rng.standard_normal((S, B)), dtype=torch.float32),
                                 h=torch.ones(B, H), c=torch.zeros(B, H), loss_buf=torch.tensor([2.5]))


def test_step_outputs_are_finite_with_the_candidate_mask_beside_the_logits():
    bench = _bench()
    rng = np.random.default_rng(5)
    shards = [_state(rng, 4, 3, 6, 8), _state(rng, 4, 2, 6, 8)]
    out = bench.step_outputs(shards[0], shards)
    assert all(np.all(np.isfinite(a)) for a in out.values())
    assert out['logits'].shape == out['logits_valid'].shape == (4, 5, 6) and out['h'].shape == (5, 8)
    full = np.concatenate([s.logits.numpy() for s in shards], 1)
    valid = out['logits_valid'].astype(bool)
    np.testing.assert_array_equal(valid, np.isfinite(full))
    np.testing.assert_array_equal(out['logits'][valid], full[valid])
    assert np.all(out['logits'][~valid] == 0)
    np.testing.assert_array_equal(out['actions'], np.concatenate([s.actions.numpy() for s in shards], 1))


def test_steps_sets_the_timed_steps_and_must_be_positive():
    bench = _bench()
    a = bench.parse(['--gpus', '1', '--steps', '7', '--warmup', '0', '--dump-outputs', 'x'])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == 'x'
    assert bench.parse([]).dump_outputs is None
    for bad in (['--steps', '0'], ['--warmup', '-1']):
        with pytest.raises(SystemExit):
            bench.parse(bad)
