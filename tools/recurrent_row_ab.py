"""The recurrent half of the decoder LSTM's gates as a row (include/sf_hip.h: sf_gate_rows_recurrent_use), ONE process,
interleaved legs, median of 7 rounds of 100 launches under the library's launch profile.
(a) The cell of one decode step alone at B rows, H = 512, LOC = 128, on caller buffers:
  - today's step: sf_lstm_cell_rows_fwd path 0, the product over [f_loc | h0], K = 640, two rows (lstm_step_wide_kernel<4>);
  - the new cell: sf_lstm_cell_rows3_fwd, the product over f_loc alone, K = 128, three rows (lstm_step_rows_kernel<1>).
(b) The product blocks launch (2) gains, xg_h = h1 W_hh^T + b_ih + b_hh, alone on launch (2)'s kernel with no scoring or
    merge blocks beside them (sf_debug_recurrent_row).  Launch (2) WITH its scoring and merge blocks, with and without the
    product blocks, is timed inside the rollout: part (c)'s per-kernel table, the same batch and the same actions in both legs.
(c) The headline rollout (100 x 20 steps, hipGraph replay, ms per rollout) with `FollowerEngine.gate_rows_recurrent` off
    and on, and -- from one eager rollout each under the launch profile -- the per-kernel times of the decode step.
    python tools/recurrent_row_ab.py [--cell-only] [B ...]"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time                                                    # noqa: E402
import torch                                                   # noqa: E402
sys.argv, ARGS = ['bench.py'], sys.argv[1:]
import bench                                                   # noqa: E402
from speaker_follower_amd import synth, features, follower     # noqa: E402
from speaker_follower_amd import _lib                          # noqa: E402
from speaker_follower_amd._lib import call, kernel_profile     # noqa: E402
from speaker_follower_amd.runtime import ptr, ws_args, stream  # noqa: E402

CELL_ONLY = '--cell-only' in ARGS
IMG, LOC, H = 2048, 128, 512
F, N = IMG + LOC, 4 * H
ROUNDS = int(os.environ.get('SF_AB_ROUNDS', '7'))


def rounds(legs, tag):
    """Interleaved: every round times each leg's 100 launches; returns {name: median us per call}."""
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
        print('%s  %s  per launch, avg of 100: median %6.2f us (rounds min %6.2f, max %6.2f)  [last round: %s]'
              % (tag, name, med[name], min(tot), max(tot), rows[name][-1][1]), flush=True)
    return med


for M in [int(a) for a in ARGS if not a.startswith('--')] or [1, 16, 17, 100]:
    dev = torch.device('cuda', 0)
    x, h0, c0 = torch.randn(M, 2 * F, device=dev), torch.randn(M, H, device=dev), torch.randn(M, H, device=dev)
    w_ih, w_hh = torch.randn(N, 2 * F, device=dev) * 0.02, torch.randn(N, H, device=dev) * 0.02
    b_ih, b_hh = torch.randn(N, device=dev) * 0.02, torch.randn(N, device=dev) * 0.02
    xg, xg2, xg_h = (torch.randn(M, N, device=dev) for _ in range(3))
    h1, c1 = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)
    w = _lib.LstmW(w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr())

    def today():
        call('sf_lstm_cell_rows_fwd', C.byref(w), M, 2 * F, H, ptr(x), 2 * F, F + IMG, ptr(xg), ptr(xg2), ptr(h0), ptr(c0),
             ptr(h1), ptr(c1), None, 0, *ws_args(dev))

    def three_rows():
        call('sf_lstm_cell_rows3_fwd', C.byref(w), M, 2 * F, H, ptr(x), 2 * F, F + IMG, ptr(xg), ptr(xg2), ptr(xg_h), ptr(h0),
             ptr(c0), ptr(h1), ptr(c1), None, *ws_args(dev))

    def product_blocks():
        call('sf_debug_recurrent_row', C.byref(w), M, H, ptr(h0), H, ptr(xg_h), stream())

    legs = (('cell, K = LOC + H = 640, two rows  ', today), ('cell, K = LOC = 128, three rows    ', three_rows),
            ('xg_h product blocks alone (K = 512)', product_blocks))
    med = rounds(legs, 'B=%3d' % M)
    print('B=%3d  the new cell saves %.2f us per step on today\'s (%.1f %%); the product blocks alone take %.2f us'
          % (M, med[legs[0][0]] - med[legs[1][0]], 100 * (med[legs[0][0]] - med[legs[1][0]]) / med[legs[0][0]],
             med[legs[2][0]]), flush=True)
if CELL_ONLY:
    sys.exit(0)

# ---- (c) the headline rollout
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


LEGS = (('recurrent half formed by the cell (gate_rows_recurrent = False)', False),
        ('recurrent half as a row of launch (2) [default]', True))
runs = {}
for name, rec in LEGS:
    eng = follower.FollowerEngine(enc, dec, store)
    eng.gate_rows_recurrent = rec
    replay, st = eng.capture(batch, 20, 'argmax')
    assert st.projected and st.gate_rows and st.gate_rows_attended and bool(st.gate_rows_recurrent) == rec
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
print('per round, off - on (ms): ' + ' '.join('%+.4f' % (a - b) for a, b in zip(runs[LEGS[0][0]][4], runs[LEGS[1][0]][4])))

for name, rec in LEGS:                       # per-kernel times of one eager rollout per leg
    eng = follower.FollowerEngine(enc, dec, store)
    eng.gate_rows_recurrent = rec
    with torch.no_grad():
        eng.rollout(batch, 20, 'argmax', train=False)
        torch.cuda.synchronize()
        with kernel_profile() as prof:
            st = eng.rollout(batch, 20, 'argmax', train=False)
            torch.cuda.synchronize()
    assert bool(st.gate_rows_recurrent) == rec
    print('\n%s: %d launches, %.1f us of kernels' % (name, sum(r['calls'] for r in prof.rows.values()),
                                                      sum(r['total_us'] for r in prof.rows.values())))
    for k, r in sorted(prof.rows.items(), key=lambda kv: -kv[1]['total_us']):
        if r['calls'] >= 18:
            print('    %-86s %3d x %6.2f us (min %.2f, max %.2f)' % (k[:86], r['calls'], r['avg_us'], r['min_us'], r['max_us']))
