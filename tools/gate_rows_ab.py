"""Gate-space rows for the action half of the decoder LSTM's input (include/sf_hip.h: sf_gate_rows_build), ONE process,
interleaved.
(a) The gate product alone, with and without the action half of the LSTM input:
[u_prev | f | h1] x [W_ih | W_hh]^T (K = 2F + H = 4864) against [f | h1] x [W_ih[:, F:] | W_hh]^T (K = F + H = 2688), what is left
of it when the action half arrives as a gate-space row (here on a dense [N, F] weight).  Both through sf_linear_slabs_fwd,
the product alone, timed by the library's launch profile.
(b) The headline rollout (100 x 20 steps, hipGraph replay, ms per rollout) on the projected chain with the rows switched off
(`FollowerEngine.gate_rows = False`) and on, the table build, and -- from one eager rollout each under the launch
profile -- the per-kernel times of the decode step.
    python tools/gate_rows_ab.py [B ...]"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time                                                    # noqa: E402
import torch                                                   # noqa: E402
sys.argv, ARGS = ['bench.py'], sys.argv[1:]
import bench                                                   # noqa: E402
from speaker_follower_amd import synth, features, follower, runtime  # noqa: E402
from speaker_follower_amd._lib import call, lib, kernel_profile       # noqa: E402
from speaker_follower_amd.runtime import ptr, ws_args          # noqa: E402

N, F, H = 2048, 2176, 512
ROUNDS = int(os.environ.get('SF_AB_ROUNDS', '7'))
for M in [int(a) for a in ARGS] or [100]:
    x, h = torch.randn(M, 2 * F).cuda(), torch.randn(M, H).cuda()
    w, u = (torch.randn(N, 2 * F) * 0.02).cuda(), (torch.randn(N, H) * 0.02).cuda()
    w1 = w[:, F:].contiguous()
    ks = C.c_int(0)

    def long_():
        call('sf_linear_slabs_fwd', ptr(x), 2 * F, ptr(w), 2 * F, ptr(h), H, ptr(u), H, M, N, C.byref(ks), *ws_args(x.device))

    def short_():
        call('sf_linear_slabs_fwd', C.c_void_p(x.data_ptr() + 4 * F), 2 * F, ptr(w1), F, ptr(h), H, ptr(u), H, M, N, C.byref(ks),
             *ws_args(x.device))

    legs = (('K = 2F + H = 4864', long_), ('K =  F + H = 2688', short_))
    rows = {name: [] for name, _ in legs}
    for fn in (long_, short_):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in legs:
            with kernel_profile() as prof:
                for _ in range(100):
                    fn()
            torch.cuda.synchronize()
            (kname, r), = [(k, v) for k, v in prof.rows.items() if 'gemm_nt' in k]
            rows[name].append((r['avg_us'], r['min_us'], r['max_us'], kname, ks.value))
    for name, _ in legs:
        avg = [r[0] for r in rows[name]]
        print('M=%3d  %s  %-28s K-split %d  avg of 100 launches: median %6.2f us (rounds min %6.2f, max %6.2f); '
              'fastest launch %6.2f us, slowest %6.2f us' % (M, name, rows[name][0][3], rows[name][0][4], statistics.median(avg),
                                                             min(avg), max(avg), min(r[1] for r in rows[name]),
                                                             max(r[2] for r in rows[name])))
    a, b = (statistics.median([r[0] for r in rows[n]]) for n, _ in legs)
    print('M=%3d  short product saves %.2f us per launch (%.1f %%)' % (M, a - b, 100 * (a - b) / a))

# ---- (b) the headline rollout
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


for label in ('first build (allocates %.2f GB)', 'rebuild in place'):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hit = store.gate_rows(dec, attended=False)
    torch.cuda.synchronize()
    gb = hit['bufs'][0].numel() * 4 / 1e9
    print('gate-space rows, %-32s %.2f ms' % ((label % gb) if '%' in label else label, 1e3 * (time.perf_counter() - t0)), flush=True)
    runtime.invalidate_caches()

LEGS = (('projected chain, full gate product (gate_rows = False)', False), ('projected chain, gate-space rows [default]', True))
runs = {}
for name, rows in LEGS:
    eng = follower.FollowerEngine(enc, dec, store)
    eng.gate_rows = rows
    eng.gate_rows_attended = False          # (the action half alone: the other half is tools/gate_rows_attended_ab.py's)
    replay, st = eng.capture(batch, 20, 'argmax')
    assert st.projected and bool(st.gate_rows) == rows
    replay()
    torch.cuda.synchronize()
    runs[name] = (replay, st, st.actions.clone(), st.logits.clone(), [])
for _ in range(ROUNDS):                      # interleaved: a drift of the box hits every leg alike
    for name, _ in LEGS:
        runs[name][4].append(timed(runs[name][0]))
base = runs[LEGS[0][0]]
for name, _ in LEGS:
    ms = runs[name][4]
    fin = torch.isfinite(base[3])
    d = float((runs[name][3][fin] - base[3][fin]).abs().max())
    scale = float(base[3][fin].abs().max())
    print('%-58s median %.4f ms per rollout (min %.4f, max %.4f; %d rounds) = %7.0f agent-steps/s, actions equal: %s, '
          'max |logit difference| %.2e (logit scale %.2f: 3e-5 * scale = %.2e)'
          % (name, statistics.median(ms), min(ms), max(ms), len(ms), 2000 / (statistics.median(ms) * 1e-3),
             bool(torch.equal(runs[name][2], base[2])), d, scale, 3e-5 * scale), flush=True)

for name, rows in LEGS:                      # per-kernel times of one eager rollout per leg
    eng = follower.FollowerEngine(enc, dec, store)
    eng.gate_rows = rows
    eng.gate_rows_attended = False          # (the action half alone: the other half is tools/gate_rows_attended_ab.py's)
    with torch.no_grad():
        eng.rollout(batch, 20, 'argmax', train=False)
        torch.cuda.synchronize()
        with kernel_profile() as prof:
            st = eng.rollout(batch, 20, 'argmax', train=False)
            torch.cuda.synchronize()
    assert bool(st.gate_rows) == rows
    print('\n%s: %d launches, %.1f us of kernels' % (name, sum(r['calls'] for r in prof.rows.values()),
                                                      sum(r['total_us'] for r in prof.rows.values())))
    for k, r in sorted(prof.rows.items(), key=lambda kv: -kv[1]['total_us']):
        if r['calls'] >= 19:
            print('    %-86s %3d x %6.2f us (min %.2f, max %.2f)' % (k[:86], r['calls'], r['avg_us'], r['min_us'], r['max_us']))
