"""Gate-space rows for the attended half of the decoder LSTM's input (include/sf_hip.h: sf_gate_rows_attended_build), ONE
process, interleaved.
(a) The cell of one decode step alone at M rows, N = 4H = 2048, through sf_lstm_cell_rows_fwd, timed by the library's launch
profile (the product and the cell kernel it needs, summed per launch of the step):
  - today's step: the action half as a gate-space row, the product over [f | h0], K = F + H = 2688, and its cell kernel;
  - both halves as rows, what is left as the two segments {LOC columns of xin, ld 2F} and {h0, W_hh, H}, K = 640, through
    the kernels csrc/sf_gemm_plan.h picks for it, and its cell kernel (which has ONE addend: this leg adds one row; the
    figures in profiles/gate_rows_attended_ab.txt were taken with a second addend in that kernel, which was not kept);
  - the same K = 640 inside the fused step kernel (lstm_step_fused: lstm_step_wide_kernel<4>), the rows as its addends.
(b) The headline rollout (100 x 20 steps, hipGraph replay, ms per rollout) with the attended rows off
(`FollowerEngine.gate_rows_attended = False`) and on, `gate_rows` on in both, the table builds, and -- from one eager
rollout each under the launch profile -- the per-kernel times of the decode step.
    python tools/gate_rows_attended_ab.py [--cell-only] [B ...]"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time                                                    # noqa: E402
import torch                                                   # noqa: E402
sys.argv, ARGS = ['bench.py'], sys.argv[1:]
import bench                                                   # noqa: E402
from speaker_follower_amd import synth, features, follower, runtime   # noqa: E402
from speaker_follower_amd import _lib                          # noqa: E402
from speaker_follower_amd._lib import call, kernel_profile     # noqa: E402
from speaker_follower_amd.runtime import ptr, ws_args          # noqa: E402

CELL_ONLY = '--cell-only' in ARGS
IMG, LOC, H = 2048, 128, 512
F, N = IMG + LOC, 4 * H
ROUNDS = int(os.environ.get('SF_AB_ROUNDS', '7'))
for M in [int(a) for a in ARGS if not a.startswith('--')] or [100]:
    dev = torch.device('cuda', 0)
    x, h0, c0 = torch.randn(M, 2 * F, device=dev), torch.randn(M, H, device=dev), torch.randn(M, H, device=dev)
    w_ih, w_hh = torch.randn(N, 2 * F, device=dev) * 0.02, torch.randn(N, H, device=dev) * 0.02
    b_ih, b_hh = torch.randn(N, device=dev) * 0.02, torch.randn(N, device=dev) * 0.02
    xg, xg2 = torch.randn(M, N, device=dev), torch.randn(M, N, device=dev)
    h1, c1 = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)
    w = _lib.LstmW(w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr())

    def cell(col0, second, path):
        def run():
            call('sf_lstm_cell_rows_fwd', C.byref(w), M, 2 * F, H, ptr(x), 2 * F, col0, ptr(xg), ptr(xg2) if second else None,
                 ptr(h0), ptr(c0), ptr(h1), ptr(c1), None, path, *ws_args(dev))
        return run

    legs = (('K =   F + H = 2688, product + cell kernel', cell(F, False, 1)),
            ('K = LOC + H =  640, product + cell kernel', cell(F + IMG, False, 1)),
            ('K = LOC + H =  640, fused step kernel    ', cell(F + IMG, True, 2)))
    rows = {name: [] for name, _ in legs}
    for _, fn in legs:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in legs:
            with kernel_profile() as prof:
                for _ in range(100):
                    fn()
            torch.cuda.synchronize()
            parts = sorted(prof.rows.items(), key=lambda kv: -kv[1]['avg_us'])
            rows[name].append((sum(r['avg_us'] for _, r in parts), ' + '.join('%s %.2f' % (k, r['avg_us']) for k, r in parts)))
    med = {}
    for name, _ in legs:
        tot = [r[0] for r in rows[name]]
        med[name] = statistics.median(tot)
        print('M=%3d  %s  per step, avg of 100: median %6.2f us (rounds min %6.2f, max %6.2f)  [last round: %s]'
              % (M, name, med[name], min(tot), max(tot), rows[name][-1][1]), flush=True)
    base = med[legs[0][0]]
    for name, _ in legs[1:]:
        print('M=%3d  %s saves %.2f us per step (%.1f %%) on today\'s' % (M, name.strip(), base - med[name],
                                                                        100 * (base - med[name]) / base), flush=True)
if CELL_ONLY:
    sys.exit(0)

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
    hit = store.gate_rows(dec)
    torch.cuda.synchronize()
    gb = (hit['bufs'][0].numel() + hit['attended']['buf'].numel()) * 4 / 1e9
    print('gate-space rows, both halves, %-32s %.2f ms' % ((label % gb) if '%' in label else label,
                                                         1e3 * (time.perf_counter() - t0)), flush=True)
    runtime.invalidate_caches()

LEGS = (('gate-space rows, action half only (gate_rows_attended = False)', False),
        ('gate-space rows, both halves [default]', True))
runs = {}
for name, att in LEGS:
    eng = follower.FollowerEngine(enc, dec, store)
    eng.gate_rows_attended = att
    replay, st = eng.capture(batch, 20, 'argmax')
    assert st.projected and st.gate_rows and bool(st.gate_rows_attended) == att
    replay()
    torch.cuda.synchronize()
    runs[name] = (replay, st, st.actions.clone(), st.logits.clone(), [])
for _ in range(ROUNDS):                      # interleaved: a drift of the machine hits every leg alike
    for name, _ in LEGS:
        runs[name][4].append(timed(runs[name][0]))
base = runs[LEGS[0][0]]
for name, _ in LEGS:
    ms = runs[name][4]
    fin = torch.isfinite(base[3])
    d = float((runs[name][3][fin] - base[3][fin]).abs().max())
    scale = float(base[3][fin].abs().max())
    print('%-64s median %.4f ms per rollout (min %.4f, max %.4f; %d rounds) = %7.0f agent-steps/s, actions equal: %s, '
          'max |logit difference| %.2e (logit scale %.2f: 3e-5 * scale = %.2e)'
          % (name, statistics.median(ms), min(ms), max(ms), len(ms), 2000 / (statistics.median(ms) * 1e-3),
             bool(torch.equal(runs[name][2], base[2])), d, scale, 3e-5 * scale), flush=True)

for name, att in LEGS:                       # per-kernel times of one eager rollout per leg
    eng = follower.FollowerEngine(enc, dec, store)
    eng.gate_rows_attended = att
    with torch.no_grad():
        eng.rollout(batch, 20, 'argmax', train=False)
        torch.cuda.synchronize()
        with kernel_profile() as prof:
            st = eng.rollout(batch, 20, 'argmax', train=False)
            torch.cuda.synchronize()
    assert bool(st.gate_rows_attended) == att
    print('\n%s: %d launches, %.1f us of kernels' % (name, sum(r['calls'] for r in prof.rows.values()),
                                                      sum(r['total_us'] for r in prof.rows.values())))
    for k, r in sorted(prof.rows.items(), key=lambda kv: -kv[1]['total_us']):
        if r['calls'] >= 19:
            print('    %-86s %3d x %6.2f us (min %.2f, max %.2f)' % (k[:86], r['calls'], r['avg_us'], r['min_us'], r['max_us']))
