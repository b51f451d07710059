"""CPU: the conditioning envelope (tests/conditioning.py) that holds the att-feed speaker's train-mode logits, and the
oracle's rounding hook and tape (oracle/torch_ref.py) it is built from.

Why an envelope.  tests/test_gpu_grads_f64.py measured the HIP path and the reference's own fp32 evaluation against
float64 and used the second as the yardstick of the first.  For the att-feed decoder in train mode (S4: B 12, 10 words,
seed 31) that yardstick is one noisy sample: the SAME fp32 computation, `torch_ref.speaker_score` on the same inputs, is

    6.2e-5  from float64 on the MI355X host   (torch at that host's default thread count, 16)
    2.29e-4 from float64 on the build machine (8 threads; worst entry: step 8, row 0)

-- a factor of four from the BLAS summation order alone.  Row 0 of that case is ill-conditioned in train mode: rounding
every operator's result once to fp32 in an otherwise exact (float64) evaluation moves its logits by up to 3.8e-4 (steps
7-8; envelope of 1 nearest + 32 random roundings, seed 1), while no other row moves by more than 3.5e-5 and eval mode by no
more than 3.2e-6 anywhere.  The envelope measures that property of the case deterministically, per (step, row), and the
bound max(1e-4, K * env) follows it; the tests below are the conditions under which that rule cannot hide a failure:
few entries get a widened bound, the rows that are well-conditioned (row 1 among them) keep the plain 1e-4, eval mode
keeps it everywhere, and the envelope does not depend on the thread count.  Numbers: profiles/att_feed_drift.txt.
"""
import numpy as np
import torch

from oracle import torch_ref
from tests import conditioning as cn
from tests import grad_compare as gc


_case = cn.s4


def _env(train):
    return cn.s4_envelope(train)[0]


def _full(case, dtype, tape=None):
    e = torch_ref.to_torch(case.senc_w, True, dtype=dtype)
    d = torch_ref.to_torch(case.sdec_w, True, frozen=('embedding.weight',), dtype=dtype)
    res = torch_ref.speaker_score(e, d, case.acts, case.feats, torch.tensor(case.path_mask), torch.tensor(case.instr_seq),
                                  case.S, 'teacher', enc_drop=case.enc_drop, dec_drop=case.dec_drop, tape=tape)
    res['loss'].backward()
    out = list(res['logits']) + [res['loss'], res['ctx'], res['h'], res['c'], res['scores']]
    return [t.detach().clone() for t in out] + [v.grad.clone() for v in list(e.values()) + list(d.values())
                                                if v.grad is not None]


def test_default_path_is_unchanged_by_the_hook_and_the_tape():
    """Hook off: outputs and gradients equal, bit for bit and in both dtypes, a run made before the hook was ever
    entered -- after a rounded run has come and gone, and with a tape attached.  Inside the hook the result does move
    (the hook is live), and an exception inside it still switches it off."""
    case = _case(True)
    for dtype in (torch.float64, torch.float32):
        before = _full(case, dtype)
        with torch_ref.rounded('nearest'):
            inside = case.run(dtype=torch.float64)
        gen = torch.Generator().manual_seed(5)
        with torch_ref.rounded('random', gen):
            case.run()
        try:
            with torch_ref.rounded('nearest'):
                raise KeyError
        except KeyError:
            pass
        tape = {}
        after = _full(case, dtype, tape)
        assert len(before) == len(after)
        for a, b in zip(before, after):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert set(tape) == {'enc', 'dec'} and len(tape['dec']['logit']) == case.S
        assert all(torch.equal(tape['dec']['logit'][t], after[t]) for t in range(case.S))
    assert not torch.equal(inside[-1], case.run()[-1])


def test_tape_names_every_intermediate():
    case = _case(True)
    tape = {}
    case.run(tape)
    B, H, F, E, Tp, S = case.B, case.dims.hidden, case.dims.feat, case.dims.word, case.Tp, case.S
    enc = {'alpha': (Tp, (B, case.dims.views)), 'feature': (Tp, (B, F)), 'concat': (Tp, (B, 2 * F)),
           'gates': (Tp, (B, 4 * H)), 'gates_act': (Tp, (B, 4 * H)), 'h': (Tp, (B, H)), 'c': (Tp, (B, H))}
    dec = {'emb': (B, E), 'h0_drop': (B, H), 'target': (B, H), 'alpha': (B, Tp), 'weighted': (B, H), 'concat': (B, E + H),
           'gates': (B, 4 * H), 'gates_act': (B, 4 * H), 'h1': (B, H), 'c1': (B, H), 'x_in': (B, 2 * H), 'x': (B, H),
           'logit': (B, case.dims.vocab)}
    assert set(tape['enc']) == set(enc) | {'decoder_init', 'ctx_raw', 'ctx'}
    for k, (n, shape) in enc.items():
        assert len(tape['enc'][k]) == n and all(tuple(v.shape) == shape for v in tape['enc'][k]), k
    assert tuple(tape['enc']['ctx'].shape) == tuple(tape['enc']['ctx_raw'].shape) == (B, Tp, H)
    assert torch.equal(tape['enc']['ctx'], tape['enc']['ctx_raw'] * case.enc_drop('ctx').double())
    assert torch.equal(tape['enc']['ctx_raw'], torch.stack(tape['enc']['h'], 1))
    assert set(tape['dec']) == set(dec)
    for k, shape in dec.items():
        assert len(tape['dec'][k]) == S and all(tuple(v.shape) == shape for v in tape['dec'][k]), k
    # the masked entries are the mask times what they mask
    t = 3
    _, d_h0, d_ht, d_x = case.dec_drop(t)
    d = tape['dec']
    assert torch.equal(d['h0_drop'][t], d['h1'][t - 1] * d_h0.double())
    assert torch.equal(d['concat'][t], torch.cat((d['emb'][t], d['weighted'][t] * d_ht.double()), 1))
    assert torch.equal(d['x_in'][t], torch.cat((d['h1'][t], d['weighted'][t]), 1) * d_x.double())


def test_rounding_modes():
    """nearest = x.float().double(); random = x (1 + d), |d| <= 2^-24, reproducible from the generator's seed."""
    x = torch.tensor([[1.0 + 2.0 ** -30, -3.0, 0.1]], dtype=torch.float64)
    w = torch.eye(3, dtype=torch.float64)
    with torch_ref.rounded('nearest'):
        y = torch_ref._linear(x, w)
    assert torch.equal(y, x.float().double()) and not torch.equal(y, x)
    outs = []
    for seed in (7, 7, 8):
        with torch_ref.rounded('random', torch.Generator().manual_seed(seed)):
            outs.append(torch_ref._linear(x, w))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    rel = ((outs[0] - x) / x).abs()
    assert float(rel.max()) <= 2.0 ** -24 and float(rel.min()) > 0
    assert torch.equal(torch_ref._linear(x, w), x)


def test_s4_train_few_entries_get_a_widened_bound():
    """At most 10% of the (step, row) pairs have K * env > 1e-4 (measured: 10 of 120; the largest, 3.8e-4, at step 8,
    row 0).  A condition, not a measurement: were most entries widened, the per-entry rule could hide a failure."""
    env = _env(True)
    wide = gc.K * env > cn.ABS_BOUND
    print('[envelope] S4 train: %d of %d pairs with K * env > 1e-4: %s; max env %.3e' % (
        wide.sum(), wide.size, ['(t %d, row %d) %.2e' % (t, r, env[t, r]) for t, r in zip(*np.nonzero(wide))], env.max()))
    assert env.shape == (10, 12)
    assert wide.sum() <= 0.10 * wide.size


def test_s4_train_well_conditioned_rows_keep_the_plain_bound():
    """Every row whose envelope stays below 2.5e-5 over all steps keeps 1e-4 at every step; row 1 -- which the open
    finding named beside row 0 -- is one of them (measured 2.30e-5), so conditioning cannot excuse it."""
    env = _env(True)
    rows = [r for r in range(env.shape[1]) if env[:, r].max() < cn.WELL_CONDITIONED]
    print('[envelope] S4 train: well-conditioned rows %s; row maxima %s' % (rows, ['%.2e' % v for v in env.max(0)]))
    assert 1 in rows
    assert 0 not in rows
    assert (cn.entry_bounds(env)[:, rows] == cn.ABS_BOUND).all()


def test_s4_eval_keeps_the_plain_bound_everywhere():
    env = _env(False)
    print('[envelope] S4 eval: max env %.3e' % env.max())
    assert gc.K * env.max() <= cn.ABS_BOUND
    assert (cn.entry_bounds(env) == cn.ABS_BOUND).all()


def test_envelope_does_not_depend_on_the_thread_count():
    """The same seed gives the same envelope on one thread and on the default count, to 1e-9 absolute (float64 summation
    order moves the rounded runs by ~1e-13) -- unlike the fp32 reference's distance, printed beside it."""
    case = _case(True)
    n = torch.get_num_threads()
    ref = case.run()
    d_n = cn.logit_distance(case.run(dtype=torch.float32), ref).max()
    torch.set_num_threads(1)
    try:
        one = cn.envelope(case.run)
        d_1 = cn.logit_distance(case.run(dtype=torch.float32), ref).max()
    finally:
        torch.set_num_threads(n)
    print('[envelope] S4 train: fp32 reference %.3e from float64 on %d threads, %.3e on 1; envelope max %.3e on both'
          % (d_n, n, d_1, one.max()))
    assert np.abs(one - _env(True)).max() <= 1e-9
    assert np.array_equal(cn.envelope(case.run, n_random=2, seed=3), cn.envelope(case.run, n_random=2, seed=3))
    assert not np.array_equal(cn.envelope(case.run, n_random=2, seed=3), cn.envelope(case.run, n_random=2, seed=4))
