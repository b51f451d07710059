"""CPU: search.BeamRecord, the record layout the two device beam searches share (include/sf_hip.h: sf_spk_beam,
sf_fol_beam), against the buffers the kernels' numpy models build by hand (test_speaker_beam_device_host.new_state,
test_follower_beam_device_host.new_state) at those models' own shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_follower_beam_device_host as FM         # noqa: E402
import test_speaker_beam_device_host as SM          # noqa: E402

SPK_PLANES = ('hist_word', 'hist_parent', 'hist_score')
FOL_PLANES = ('parent', 'action', 'rank', 'sid', 'psid', 'score')


def by_hand(model, B, beam, steps, n_planes, width):
    """Offsets, header length and per-step stride from the sizes of the model's own arrays, laid end to end in the
    order of the contract: inst, live_total, done_rec, done_score, padding to 4 words; per step the planes of R words,
    then the attention."""
    R = B * beam
    assert model['live_total'].size == steps and model['inst'].shape == (B, 3)
    o_live = model['inst'].size
    o_done = o_live + model['live_total'].size
    o_dscore = o_done + model['done_rec'].size
    end = o_dscore + model['done_score'].size
    return dict(o_live=o_live, o_done=o_done, o_dscore=o_dscore, hdr=-(-end // 4) * 4, stride=n_planes * R + R * width)


def check(rec, want, steps):
    for name, v in want.items():
        assert getattr(rec, name) == v, name
    assert rec.size == want['hdr'] + steps * want['stride']
    head = rec.head0()
    assert head.dtype == np.int32 and head.shape == (want['hdr'],)
    assert (head[:want['o_live']].reshape(-1, 3) == (1, 0, 0)).all() and not head[want['o_live']:].any()
    # device pointers: byte addresses of the same offsets, in the order of the structs' fields
    base = 1 << 20
    p = rec.pointers(base)
    words = [(x - base) // 4 for x in p[:2] + p[2:-3] + p[-2:]]
    n = len(rec.planes)
    assert words == ([0, want['o_live']] + [want['hdr'] + j * rec.R for j in range(n + 1)]
                     + [want['o_done'], want['o_dscore']])
    assert p[-3] == want['stride'] and all((x - base) % 4 == 0 for x in p[:-3] + p[-2:])


def check_split(rec, attn, t_end):
    """A record filled with arange (and t = t_end in every instance's header) comes apart at the documented places."""
    B, R, W2, n = rec.B, rec.R, 2 * rec.beam, len(rec.planes)
    flat = np.arange(rec.size, dtype=np.int32)
    flat[2:3 * B:3] = t_end
    out = rec.split(flat, attn=attn)
    assert set(out) == {'inst', 'done_rec', 'done_score', attn, *rec.planes}
    assert np.array_equal(out['inst'], flat[:3 * B].reshape(B, 3))
    assert np.array_equal(out['done_rec'], (rec.o_done + np.arange(B * W2)).reshape(B, W2))
    assert out['done_score'].dtype == np.float32
    assert np.array_equal(out['done_score'].view(np.int32), (rec.o_dscore + np.arange(B * W2)).reshape(B, W2))
    step0 = rec.hdr + rec.stride * np.arange(t_end)[:, None]
    for j, name in enumerate(rec.planes):
        got = out[name]
        assert got.shape == (t_end, R)
        assert got.dtype == (np.float32 if j == n - 1 else np.int32), name
        assert np.array_equal(got.view(np.int32), step0 + j * R + np.arange(R)), name
    a = out[attn]
    assert a.dtype == np.float32 and a.shape == (t_end, R, rec.width)
    assert np.array_equal(a.view(np.int32).reshape(t_end, -1), step0 + n * R + np.arange(R * rec.width))


@pytest.mark.parametrize('B,beam,T,Tp', [(3, 4, 6, 4), (2, 1, 5, 4)])
def test_speaker_record_is_the_models_layout(B, beam, T, Tp):
    from speaker_follower_amd.search import BeamRecord
    rec = BeamRecord(B, beam, T, SPK_PLANES, Tp)
    model = SM.new_state(B, beam, T, Tp)
    assert all(model[name].shape[0] == T for name in SPK_PLANES + ('hist_attn',))
    check(rec, by_hand(model, B, beam, T, len(SPK_PLANES), Tp), T)
    check_split(rec, 'hist_attn', T - 1)
    assert set(SM.history_of(model)) == set(rec.split(np.zeros(rec.size, np.int32), attn='hist_attn'))


@pytest.mark.parametrize('B,beam,E,T', [(3, 4, 6, 5), (2, 1, 5, 5)])
def test_follower_record_is_the_models_layout(B, beam, E, T):
    from speaker_follower_amd.search import BeamRecord, DeviceFollowerBeam
    assert DeviceFollowerBeam.PLANES == FOL_PLANES
    rec = BeamRecord(B, beam, E, FOL_PLANES, T)
    model = FM.new_state(B, beam, E, T, np.zeros(B, np.int64))
    assert all(model['hist_' + name].shape == (E, B * beam) for name in FOL_PLANES)
    assert model['hist_attn'].shape == (E, B * beam, T)
    check(rec, by_hand(model, B, beam, E, len(FOL_PLANES), T), E)
    check_split(rec, 'attn', E - 1)
    assert set(FM.history_of(model)) == set(rec.split(np.zeros(rec.size, np.int32)))
