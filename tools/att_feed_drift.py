#!/usr/bin/env python3
"""The att-feed speaker's train-mode logits (S4 of tests/test_gpu_grads_f64.py: B 12, 10 words) against float64 under one
of the switches that change the arithmetic of the module path, one switch per process:

    python tools/att_feed_drift.py default      as the suite runs it
    python tools/att_feed_drift.py strict       sf_gate_product_strict(1): the M <= 128 gate products off the bf16x6 split
    python tools/att_feed_drift.py noprecise    sf_debug_precise_attention(0): the engines' visual attention in fp32 (the
                                                module path's sf_visual_attention_fwd_f64 does not read the switch)

Prints the largest distance, where it is, the per-row maxima, and the conditioning envelope (tests/conditioning.py) beside
them.  GPU.  profiles/att_feed_drift.txt records a run.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speaker_follower_amd import _lib                                  # noqa: E402
from tests import conditioning as cn                                   # noqa: E402
import tests.test_gpu_grads_f64 as grads                               # noqa: E402


def main(mode):
    if mode == 'strict':
        _lib.lib.sf_gate_product_strict(1)
    elif mode == 'noprecise':
        _lib.lib.sf_debug_precise_attention(0)
    elif mode != 'default':
        raise SystemExit(__doc__)
    c = grads._s4(True)
    ref = c['r64']['logits']
    got = [c['logits'][t][:, :ref[t].shape[1]] for t in range(c['n'])]
    d = cn.logit_distance(got, ref)
    d32 = cn.logit_distance(c['r32']['logits'], ref)
    env, _ = cn.s4_envelope(True)
    bound = cn.entry_bounds(env)
    t, r = np.unravel_index(np.argmax(d), d.shape)
    print('[%s] max |dlogit| %.3e at (step %d, row %d), env there %.3e; row 1 %.3e; rows 1-11 %.3e; worst d / bound %.2f; '
          'entries outside their bound %d of %d; the fp32 reference %.3e (%d threads)'
          % (mode, d.max(), t, r, env[t, r], d[:, 1].max(), d[:, 1:].max(), (d / bound).max(), int((d > bound).sum()),
             d.size, d32.max(), torch.get_num_threads()))
    print('[%s] per-row max |dlogit| %s' % (mode, ' '.join('%.2e' % v for v in d.max(0))))
    print('[%s] per-row max env      %s' % (mode, ' '.join('%.2e' % v for v in env.max(0))))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'default')
