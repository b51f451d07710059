"""A/B of the projected decode chain on the headline batch (100 x 20 steps, hipGraph replay, ms per rollout), both
chains in ONE process, interleaved: the four-launch folded chain (project = False), the projected chain with the attention
partials in launch (1) (the default) and with the partials in launch (2) (sf_debug_projected_partials_late(1)) -- and
launch (1) with four text groups per sample forced (sf_debug_projected_text_groups(4)) against the library's rule
(two groups where the four-group grid does not fit the device at once: this batch).
Reports median / min / max over the rounds, the table build, and -- from one eager rollout each under the library's launch
profile -- the per-kernel times of the decode step."""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
sys.argv = ['bench.py']
import bench
from speaker_follower_amd import synth, features, follower, _lib
ROUNDS = int(os.environ.get('SF_AB_ROUNDS', '7'))
DEFAULT_LATE = 0         # csrc/sf_api.hip: sf_debug_projected_partials_late
dev = torch.device('cuda', 0)
enc, dec, _, _ = bench.build_models(101, dev)
enc.eval(); dec.eval()
store = features.FeatureStore(bench.device_table(10567, 1234, dev), device=dev)
fb = synth.follower_batch(seed=0, batch=100, steps=20, n_viewpoints=10567)
batch = follower.DeviceFollowerBatch.from_synth(fb, device=dev)


def timed(replay, n=40):
    for _ in range(8):
        replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        replay()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


# the table build: the first one allocates, the second (forced by the invalidation epoch) rebuilds in place
from speaker_follower_amd import runtime
for label in ('first build (allocates 2 x %.2f GB)', 'rebuild in place'):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hit = store.projected(dec)
    torch.cuda.synchronize()
    gb = hit['bufs'][0].numel() * 4 / 1e9
    print('projected tables, %-36s %.2f ms' % ((label % gb) if '%' in label else label, 1e3 * (time.perf_counter() - t0)), flush=True)
    runtime.invalidate_caches()

LEGS = (('folded, four launches (project = False)', False, 0, 0),
        ('projected, partials in launch (2)', True, 1, 0),
        ('projected, partials in (1), four text groups', True, 0, 4),
        ('projected, partials in (1), rule [default]', True, 0, 0))
runs = {}
for name, project, late, groups in LEGS:
    _lib.lib.sf_debug_projected_partials_late(late)
    _lib.lib.sf_debug_projected_text_groups(groups)
    eng = follower.FollowerEngine(enc, dec, store)
    eng.project = project
    replay, st = eng.capture(batch, 20, 'argmax')
    assert bool(st.projected) == bool(project)
    replay()
    torch.cuda.synchronize()
    runs[name] = (replay, st, st.actions.clone(), st.logits.clone(), [])
_lib.lib.sf_debug_projected_partials_late(DEFAULT_LATE)
_lib.lib.sf_debug_projected_text_groups(0)
for _ in range(ROUNDS):                      # interleaved: a drift of the box hits every leg alike
    for name, _, _, _ in LEGS:
        runs[name][4].append(timed(runs[name][0]))
base = runs[LEGS[0][0]]
for name, _, _, _ in LEGS:
    ms = runs[name][4]
    fin = torch.isfinite(base[3])
    d = float((runs[name][3][fin] - base[3][fin]).abs().max())
    scale = float(base[3][fin].abs().max())
    print('%-44s median %.4f ms per rollout (min %.4f, max %.4f; %d rounds) = %7.0f agent-steps/s, actions equal: %s, '
          'max |logit difference| %.2e (logit scale %.2f: 3e-5 * scale = %.2e)'
          % (name, statistics.median(ms), min(ms), max(ms), len(ms), 2000 / (statistics.median(ms) * 1e-3),
             bool(torch.equal(runs[name][2], base[2])), d, scale, 3e-5 * scale), flush=True)

# per-kernel times of one eager rollout per leg (the launches of the 20 decode steps and what surrounds them)
for name, project, late, groups in LEGS:
    _lib.lib.sf_debug_projected_partials_late(late)
    _lib.lib.sf_debug_projected_text_groups(groups)
    eng = follower.FollowerEngine(enc, dec, store)
    eng.project = project
    with torch.no_grad():
        eng.rollout(batch, 20, 'argmax', train=False)
        torch.cuda.synchronize()
        with _lib.kernel_profile() as prof:
            eng.rollout(batch, 20, 'argmax', train=False)
            torch.cuda.synchronize()
    print('\n%s: %d launches, %.1f us of kernels' % (name, sum(r['calls'] for r in prof.rows.values()),
                                                      sum(r['total_us'] for r in prof.rows.values())))
    for k, r in sorted(prof.rows.items(), key=lambda kv: -kv[1]['total_us']):
        if r['calls'] >= 19:
            print('    %-86s %3d x %6.2f us (min %.2f, max %.2f)' % (k[:86], r['calls'], r['avg_us'], r['min_us'], r['max_us']))
_lib.lib.sf_debug_projected_partials_late(DEFAULT_LATE)
_lib.lib.sf_debug_projected_text_groups(0)
