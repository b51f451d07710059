"""CPU: the element-wise gradient comparator (tests/grad_compare.py) closes the gap of the older end-to-end check
(L2 norm + 16 sampled entries at rtol 3e-3, `norm_sample_check`).  Synthetic gradient sets shaped like the follower
decoder's (LSTM weight_ih over [u_prev features | u_prev location | attended features | attended location]) and an
embedding table, each with one localised corruption a training-gradient bug would leave: the older check accepts every
one of them (for every sample draw tried), the comparator rejects every one and accepts the uncorrupted set."""
import numpy as np
import pytest

from tests import grad_compare as gc

H, FI, FL, V, E, S, B = 64, 256, 16, 991, 32, 20, 40
K_IH = 2 * (FI + FL)
SEGS = [('u_feat', 0, FI), ('u_loc', FI, FI + FL), ('att_feat', FI + FL, 2 * FI + FL), ('att_loc', 2 * FI + FL, K_IH)]


def _stack_sum(x, d):
    return np.einsum('sbk,sbh->hk', x, d)


def _sets():
    """(per-step pieces, reference gradients): weight_ih = sum over S steps of dgates^T x (ragged: rows stop at their
    own length), its location columns and the f gate an order of magnitude smaller than the rest (as in the follower:
    location features and the forget gate's gradient are small), an embedding gradient with a padding row and absent
    tokens."""
    r = np.random.default_rng(0)
    lens = r.integers(2, S, size=B)
    lens[0] = S                                                  # one row reaches the last step ...
    live = (np.arange(S)[:, None] < lens[None, :]).astype(np.float64)
    x = r.standard_normal((S, B, K_IH))
    x[:, :, FI:FI + FL] *= 0.05
    x[:, :, 2 * FI + FL:] *= 0.05
    d = r.standard_normal((S, B, 4 * H)) * live[:, :, None]
    d[:, :, H:2 * H] *= 0.1
    d[S - 1] *= 0.01                                             # ... with a confident (small-gradient) prediction
    w_ih = _stack_sum(x, d)
    bias = d.sum((0, 1))
    emb = np.zeros((V, E))
    toks = r.integers(4, V, size=S * B)                        # tokens 0 (padding) .. 3 and some others never occur
    np.add.at(emb, toks, r.standard_normal((S * B, E)))
    lin_out = r.standard_normal((H, 2 * H))
    ref = {'lstm.weight_ih': w_ih, 'lstm.bias_ih': bias, 'embedding.weight': emb,
           'text_attention_layer.linear_out.weight': lin_out,
           'decoder2action.linear_out.bias': np.array([1e-17])}
    return (x, d, live), ref


def _blocks():
    return {'lstm.weight_ih': gc.lstm_blocks(4 * H, SEGS), 'lstm.bias_ih': gc.lstm_blocks(4 * H),
            'embedding.weight': gc.row_blocks(V),
            'text_attention_layer.linear_out.weight': gc.halves_blocks(2 * H, H)}


def _noisy(ref, rel, seed):
    """ref + roundoff-like noise: `rel` x each element's magnitude (+ 1e-3 of the tensor's max)."""
    r = np.random.default_rng(seed)
    out = {}
    for k, v in ref.items():
        out[k] = v + rel * (np.abs(v) + 1e-3 * np.abs(v).max()) * r.standard_normal(v.shape) * (v != 0)
    return out


def _corrupt(kind, pieces, hip):
    x, d, live = pieces
    hip = {k: v.copy() for k, v in hip.items()}
    w = hip['lstm.weight_ih']
    if kind == 'one gate block off by 1%':
        w[H:2 * H] *= 1.01
    elif kind == 'location columns off by 2%':
        w[:, FI:FI + FL] *= 1.02
        w[:, 2 * FI + FL:] *= 1.02
    elif kind == 'one embedding row wrong':
        e = hip['embedding.weight']
        row = int(np.argmax(np.abs(e).sum(1)))
        e[row] = e[row][::-1]
    elif kind == "last step's rows missing from the stacked sum":
        hip['lstm.weight_ih'] = w - _stack_sum(x[S - 1:], d[S - 1:])
    elif kind == 'padding row not zero':
        hip['embedding.weight'][0, 3] = 1e-30
    else:
        raise ValueError(kind)
    return hip


KINDS = ['one gate block off by 1%', 'location columns off by 2%', 'one embedding row wrong',
         "last step's rows missing from the stacked sum", 'padding row not zero']


def test_comparator_accepts_roundoff():
    pieces, ref = _sets()
    rep = gc.compare_grads(_noisy(ref, 2e-7, 1), ref, _noisy(ref, 1e-7, 2), _blocks(), what='synthetic')
    name, e, e32 = rep.worst()
    assert e < 1e-5 and e32 < 1e-5


@pytest.mark.parametrize('kind', KINDS)
def test_old_check_accepts_what_the_comparator_rejects(kind):
    pieces, ref = _sets()
    hip = _corrupt(kind, pieces, _noisy(ref, 2e-7, 1))
    assert any(np.any(hip[k] != v) for k, v in _noisy(ref, 2e-7, 1).items())
    for seed in range(8):                                    # the older check passes whatever 16 entries it samples
        gc.norm_sample_check(hip, ref, np.random.default_rng(seed))
    with pytest.raises(AssertionError):
        gc.compare_grads(hip, ref, _noisy(ref, 1e-7, 2), _blocks(), what='synthetic (%s)' % kind)


def test_exact_zero_gradient_rule():
    _, ref = _sets()
    hip = _noisy(ref, 2e-7, 1)
    hip['decoder2action.linear_out.bias'] = np.array([1e-3])
    with pytest.raises(AssertionError, match='exact gradient is zero'):
        gc.compare_grads(hip, ref, _noisy(ref, 1e-7, 2), _blocks())


def test_tensor_bound_follows_the_reference_fp32_drift():
    """e is bounded by K x e32 above the floor, and never by more than the ceiling."""
    _, ref = _sets()
    f32 = _noisy(ref, 1e-5, 2)
    gc.compare_grads(_noisy(ref, 3e-5, 1), ref, f32, what='drift')          # e ~ 3 e32: inside K = 4
    with pytest.raises(AssertionError):
        gc.compare_grads(_noisy(ref, 3e-4, 1), ref, f32, what='drift')      # e ~ 30 e32
    with pytest.raises(AssertionError, match='ceiling'):
        gc.compare_grads(_noisy(ref, 2e-4, 1), ref, _noisy(ref, 1e-4, 2), what='drift')
