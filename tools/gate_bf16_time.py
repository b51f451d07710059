"""The decode gate product with fp32 and with bf16-stored weights (runtime.bf16_gate_weights / FollowerEngine.gate_weights),
both in ONE process after a warm-up, alternating:

  * the gate-product launch alone at M = 100 ([100, 4352 | 512] x [2048, 4352 | 512]^T through sf_linear_slabs_fwd): kernel
    time from the library's own launch events (kernel_profile), median / min / max over the timed launches;
  * the headline-shape rollout (B = 100, 20 steps, encoder included) as a replayed hipGraph per mode: median / min / max of
    BLOCKS timed blocks of REPLAYS replays each, the two modes interleaved block by block.

The comparison is always against the fp32-weights path of the same run.  Prints one JSON line at the end.
    python tools/gate_bf16_time.py [--blocks 12] [--replays 40]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_argv, sys.argv = sys.argv, ['bench.py']
import bench                                                            # noqa: E402
sys.argv = _argv
from speaker_follower_amd import synth, features, follower, runtime    # noqa: E402
from speaker_follower_amd._lib import call, kernel_profile, lib         # noqa: E402
from speaker_follower_amd.runtime import ptr, ws_args                   # noqa: E402


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def product_times(dev, launches):
    """Kernel time (us) of the gate-product launch at M = 100 per mode: launches alternate between the modes."""
    M, N, K1, K2 = 100, 2048, 4352, 512
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(M, K1, generator=g) * 0.5 + 0.4).to(dev)
    h = torch.tanh(torch.randn(M, K2, generator=g)).to(dev)
    w, u = (torch.randn(N, K1, generator=g) * 0.03).to(dev), (torch.randn(N, K2, generator=g) * 0.05).to(dev)
    assert lib.sf_gate_product_bf16_supported(M, K1, K2, N) == 1
    runtime.register_bf16_weights(w, u)
    ks = C.c_int(0)

    def launch():
        call('sf_linear_slabs_fwd', ptr(x), K1, ptr(w), K1, ptr(h), K2, ptr(u), K2, M, N, C.byref(ks), *ws_args(dev))
    out = {'fp32': [], 'bf16': []}
    names = {}
    for i in range(launches + 8):
        for mode in ('fp32', 'bf16'):
            with runtime.bf16_gate_weights(mode == 'bf16'):
                with kernel_profile() as prof:
                    launch()
            torch.cuda.synchronize()
            (name, row), = prof.rows.items()
            names[mode] = name
            if i >= 8:                                                   # (warm-up: code objects, caches, clocks)
                out[mode].append(row['total_us'])
    return {m: dict(spread(v), kernel=names[m]) for m, v in out.items()}


def rollout_times(dev, blocks, replays):
    """Milliseconds per replayed rollout (B = 100, 20 steps, encoder included) per mode, blocks interleaved."""
    enc, dec, _, _ = bench.build_models(101, dev)
    enc.eval()
    dec.eval()
    store = features.FeatureStore(bench.device_table(10567, 1234, dev), device=dev)
    fb = synth.follower_batch(seed=0, batch=100, steps=20, n_viewpoints=10567)
    batch = follower.DeviceFollowerBatch.from_synth(fb, device=dev)
    runs = {}
    for mode in ('fp32', 'bf16'):
        eng = follower.FollowerEngine(enc, dec, store)
        eng.gate_weights = mode
        runs[mode] = eng.capture(batch, 20, 'argmax')
    with torch.no_grad():                                                # the per-kernel view of one eager rollout per mode
        kernels = {}
        for mode in ('fp32', 'bf16'):
            eng = follower.FollowerEngine(enc, dec, store)
            eng.gate_weights = mode
            eng.rollout(batch, 20, 'argmax', train=False)
            with kernel_profile() as prof:
                eng.rollout(batch, 20, 'argmax', train=False)
            torch.cuda.synchronize()
            gate = {k: v for k, v in prof.rows.items() if 'gemm_nt_split' in k or 'gemm_nt_bf16w' in k}
            kernels[mode] = dict(total_us=sum(v['total_us'] for v in prof.rows.values()),
                                 gate={k: dict(calls=v['calls'], avg_us=v['avg_us']) for k, v in gate.items()})
    times = {'fp32': [], 'bf16': []}
    for blk in range(blocks + 2):
        for mode in ('fp32', 'bf16'):
            replay = runs[mode][0]
            for _ in range(5):
                replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replays):
                replay()
            torch.cuda.synchronize()
            if blk >= 2:
                times[mode].append(1e3 * (time.perf_counter() - t0) / replays)
    a, b = (runs[m][1] for m in ('fp32', 'bf16'))
    same = int((a.actions == b.actions).sum())
    dl = float((a.logits - b.logits)[torch.isfinite(a.logits)].abs().max())
    return ({m: spread(v) for m, v in times.items()}, kernels,
            dict(equal_actions=same, of=a.actions.numel(), max_dlogit=dl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=12)
    ap.add_argument('--replays', type=int, default=40)
    ap.add_argument('--launches', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gate_bf16_time.py measures on a GPU: none found')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    prod = product_times(dev, args.launches)
    roll, kernels, diff = rollout_times(dev, max(12, args.blocks), args.replays)
    for name, t, unit in (('gate product M=100', prod, 'us'), ('rollout B=100 x 20', roll, 'ms')):
        for m in ('fp32', 'bf16'):
            print('%-20s %s weights: median %.3f  min %.3f  max %.3f %s (n = %d)'
                  % (name, m, t[m]['median'], t[m]['min'], t[m]['max'], unit, t[m]['n']))
        faster = t['bf16']['median'] < t['fp32']['min']
        print('%-20s bf16 median %s the fp32 minimum: %s' % (name, 'below' if faster else 'NOT below',
                                                            'faster' if faster else 'not counted as faster'))
    print(json.dumps(dict(gate_product_us=prod, rollout_ms=roll, eager_kernels=kernels, fp32_vs_bf16=diff)))


if __name__ == '__main__':
    main()
