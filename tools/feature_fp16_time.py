"""The headline rollout (B = 100, 20 steps, 10 567-viewpoint table, encoder included) on an fp32 and on an fp16 feature
store (features.FeatureStore(dtype=...)), both in ONE process after a warm-up, alternating:

  * the rollout as a replayed hipGraph per store: median / min / max of BLOCKS timed blocks of REPLAYS replays each, the two
    stores interleaved block by block (a host clock around work that ends in a device synchronise);
  * per store, the per-launch kernel time of the launches that read table rows -- pair_vis_small_kernel (the panorama
    partials) and the scoring launch -- from the library's own launch events (kernel_profile) over one eager rollout;
  * the bytes those launches must move, computed from the shapes.

The comparison is always against the fp32 store of the same run.  Prints one JSON line at the end.
    python tools/feature_fp16_time.py [--blocks 12] [--replays 40]
"""
import argparse
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
from speaker_follower_amd import synth, features, follower             # noqa: E402
from speaker_follower_amd._lib import kernel_profile                    # noqa: E402

TABLE_KERNELS = ('pair_vis_small_kernel', 'visual_attn', 'score', 'follower_glue')


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=12)
    ap.add_argument('--replays', type=int, default=40)
    ap.add_argument('--viewpoints', type=int, default=10567)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feature_fp16_time.py measures on a GPU: none found')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    B, S, NVP = 100, 20, args.viewpoints
    enc, dec, _, _ = bench.build_models(101, dev)
    enc.eval()
    dec.eval()
    table = bench.device_table(NVP, 1234, dev)
    stores = {'fp32': features.FeatureStore(table, device=dev),
              'fp16': features.FeatureStore(table, device=dev, dtype='fp16')}
    fb = synth.follower_batch(seed=0, batch=B, steps=S, n_viewpoints=NVP)
    batch = follower.DeviceFollowerBatch.from_synth(fb, device=dev)
    V, IMG, LOC = stores['fp32'].V, stores['fp32'].IMG, stores['fp32'].LOC
    # bytes per launch, from the shapes: the panorama launch reads every sample's V rows (image part from the table, location
    # part from the fp32 location table); the scoring launch reads one image row per live candidate (none for stop / padding)
    live = int(sum(int(fb.a_num[t, b]) - 1 for t in range(S) for b in range(B))) / S
    nbytes = {m: dict(panorama_MB=B * V * (IMG * w + LOC * 4) / 1e6, scoring_MB=live * IMG * w / 1e6,
                      table_GB=stores[m].table.numel() * stores[m].table.element_size() / 1e9)
              for m, w in (('fp32', 4), ('fp16', 2))}

    runs, kernels = {}, {}
    for m, store in stores.items():
        runs[m] = follower.FollowerEngine(enc, dec, store).capture(batch, S, 'argmax')
    with torch.no_grad():                                                # the per-kernel view of one eager rollout per store
        for m, store in stores.items():
            eng = follower.FollowerEngine(enc, dec, store)
            eng.rollout(batch, S, 'argmax', train=False)
            with kernel_profile() as prof:
                eng.rollout(batch, S, 'argmax', train=False)
            torch.cuda.synchronize()
            kernels[m] = dict(total_us=sum(v['total_us'] for v in prof.rows.values()),
                              table_launches={k: dict(calls=v['calls'], avg_us=v['avg_us']) for k, v in prof.rows.items()
                                              if any(n in k for n in TABLE_KERNELS)})
    times = {m: [] for m in stores}
    for blk in range(args.blocks + 2):
        for m in stores:
            replay = runs[m][0]
            for _ in range(5):
                replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.replays):
                replay()
            torch.cuda.synchronize()
            if blk >= 2:                                                 # (warm-up: code objects, caches, clocks)
                times[m].append(1e3 * (time.perf_counter() - t0) / args.replays)
    roll = {m: spread(v) for m, v in times.items()}
    a, b = (runs[m][1] for m in ('fp32', 'fp16'))
    fin = torch.isfinite(a.logits) & torch.isfinite(b.logits)
    diff = dict(equal_actions=int((a.actions == b.actions).sum()), of=a.actions.numel(),
                max_dlogit=float((a.logits - b.logits)[fin].abs().max()))
    for m in ('fp32', 'fp16'):
        t = roll[m]
        print('rollout B=%d x %d, %s store: median %.3f  min %.3f  max %.3f ms (n = %d); table %.2f GB, panorama launch '
              '%.1f MB, scoring launch %.1f MB' % (B, S, m, t['median'], t['min'], t['max'], t['n'], nbytes[m]['table_GB'],
                                                  nbytes[m]['panorama_MB'], nbytes[m]['scoring_MB']))
        for k, v in sorted(kernels[m]['table_launches'].items()):
            print('    %-60s %4d launches, %8.2f us each' % (k[:60], v['calls'], v['avg_us']))
    faster = roll['fp16']['median'] < roll['fp32']['min']
    print('fp16 median %s the fp32 minimum: %s' % ('below' if faster else 'NOT below',
                                                   'faster' if faster else 'not counted as faster'))
    print(json.dumps(dict(rollout_ms=roll, bytes=nbytes, eager_kernels=kernels, fp32_vs_fp16=diff)))


if __name__ == '__main__':
    main()
