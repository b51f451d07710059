"""GPU, end to end: Seq2SeqSpeaker.test() with `device_routes` -- the split's packed minibatches written by sf_nav_routes
on the device, one D2D copy and one replay per minibatch -- against the same test() with the switch off (gold_routes +
pack_speaker_batch + one H2D copy per minibatch).  The staging bytes are equal (tests/test_gpu_nav_routes.py), the
graphs are the same, so words, scores and losses are compared with ==.  A speaker with the peaky weights of the
persistent-launch tests over the eight committed scans; `sweep_test_after = 0`."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nav_route_cases as R                                         # noqa: E402
from speaker_follower_amd import synth                              # noqa: E402

INSTRUCTION_LEN, EPISODE_LEN = 14, 10


@pytest.fixture(scope='module')
def world():
    from speaker_follower_amd import features, model
    from speaker_follower_amd.routes import RouteSet
    state = random.getstate()
    env, nav, dist, n_rows = R.fixture_world('cuda')
    d = synth.FULL
    w_enc, w_dec = synth.speaker_weights_peaky(404)
    enc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    dec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=w_dec['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in w_enc.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in w_dec.items()})
    store = features.FeatureStore(synth.feature_table(21, n_rows))
    yield dict(base=env, nav=nav, routes=RouteSet.enumerate(nav, dist), enc=enc.cuda().eval(), dec=dec.cuda().eval(), store=store)
    random.setstate(state)


def speaker_over(world, items, B):
    """A fresh speaker (its own sweep and graphs) over an env of `items` in minibatches of B."""
    from speaker_follower_amd import agents, env as E
    base = world['base']
    env = E.R2RIndexEnv(items, base.row_of, base.nav_graph_path, batch_size=B, scans=world['nav'].scans)
    spk = agents.Seq2SeqSpeaker(env, '/tmp/sf_speaker_routes.json', world['enc'], world['dec'], INSTRUCTION_LEN,
                                max_episode_len=EPISODE_LEN)
    spk.store = world['store']
    spk.sweep_test_after = 0
    return spk, env


def run_test(spk, env, device_routes, chunk=None):
    """test() from the same item order and the same state of `random` (the epoch wraps inside test())."""
    spk.device_routes, spk.device_routes_chunk = device_routes, chunk
    random.seed(17)
    env.data.sort(key=lambda it: it['instr_id'])
    res = spk.test(use_dropout=False, feedback='argmax')
    return ({k: (list(v['word_indices']), v['score'], list(v['scores'])) for k, v in res.items()}, list(spk.losses),
            [it['instr_id'] for it in env.batch])


def fixture_split(world):
    fx = json.load(open(os.path.join(HERE, 'golden', 'r2r_fixture_items.json')))['items']
    return [dict(it, instr_encoding=np.asarray(it['instr_encoding'], np.int64)) for it in fx]


def test_device_routes_equal_the_host_path_on_whole_multiples_of_the_batch(world, monkeypatch):
    from speaker_follower_amd.routes import RouteSet
    items = world['routes'].sample(200, 7).items()
    spk, env = speaker_over(world, items, 20)
    # switch off: nothing of the feature runs, the host packs as before
    with monkeypatch.context() as m:
        m.setattr(RouteSet, 'pack', lambda *a, **k: pytest.fail('RouteSet.pack with device_routes off'))
        off = run_test(spk, env, False)
    sweep = spk._test_sweep[1]
    assert sweep.host_pack_s > 0 and sweep.fallbacks == 0 and len(off[0]) == 200
    assert len(off[1]) == 11                                          # (ten minibatches, and the one in which test() sees the wrap)
    graphs = len(sweep.graphs)
    on = run_test(spk, env, True)
    assert spk._test_sweep[1] is sweep and len(sweep.graphs) == graphs        # the graphs of the same step counts, replayed
    assert sweep.host_pack_s == 0.0 and sweep.fallbacks == 0
    assert on == off                                                  # words, score, scores, losses, the last minibatch
    assert len({tuple(v[0]) for v in on[0].values()}) > 20            # (the routes do decide the words)
    assert run_test(spk, env, True, chunk=2) == off                   # five device buffers instead of one
    # the fixture split: real instruction encodings (they fill instr_seq; argmax decoding does not read them)
    split = fixture_split(world)
    B = max(b for b in range(2, 21) if len(split) % b == 0)
    spk, env = speaker_over(world, split, B)
    off = run_test(spk, env, False)
    assert run_test(spk, env, True) == off and len(off[0]) == len(split) and len(off[1]) == len(split) // B + 1


def test_device_routes_on_a_ragged_split(world):
    """N % B != 0: the last minibatch is filled by the environment from the reshuffled split; first occurrences count."""
    items = world['routes'].sample(50, 9).items()
    spk, env = speaker_over(world, items, 20)
    off = run_test(spk, env, False)
    on = run_test(spk, env, True)
    assert len(off[0]) == 50 and len(off[1]) == 3 and on == off


def test_augment_equals_test_over_the_env_of_the_routes_items(world):
    rs = world['routes'].sample(120, 11)
    spk, env = speaker_over(world, rs.items(), 40)
    want = run_test(spk, env, False)
    env.data.sort(key=lambda it: it['instr_id'])                      # the order test() walked (120 = 3 x 40: no wrap)
    at = {'%d_0' % p: i for i, p in enumerate(rs.path_ids)}
    ordered = rs.take([at[it['instr_id']] for it in env.data])
    spk.env = None                                                    # no environment involved
    got = spk.augment(ordered, batch_size=40)
    assert list(got) == [it['instr_id'] for it in env.data]
    assert {k: (list(v['word_indices']), v['score'], list(v['scores'])) for k, v in got.items()} == want[0]
    assert list(spk.losses) == want[1][:3]                            # (test() draws a fourth minibatch to see the wrap)
    replaced = ordered.replaced_items(got)
    assert [r['path_id'] for r in replaced] == sorted(int(p) for p in rs.path_ids)
    by_id = {it['path_id']: it for it in rs.items()}
    for r in replaced:
        assert r == dict(by_id[r['path_id']], instructions=[' '.join(str(w) for w in got['%d_0' % r['path_id']]['words'])])
    # a short last minibatch is filled from the front: every route once, the same words for all but that minibatch
    ragged = spk.augment(ordered.take(np.arange(100)), batch_size=40)
    assert list(ragged) == list(got)[:100]
    assert all(list(ragged[k]['word_indices']) == want[0][k][0] for k in list(got)[:80])


def test_a_starved_sweep_is_reissued_from_the_same_device_blocks(world):
    """Every persistent word loop of the sweep gives up its first wait (the existing injection switch, set while the
    graphs are captured): `finish` re-runs the sweep on the per-step graphs from the SAME PackedBlocks."""
    from speaker_follower_amd import _lib, runtime
    items = world['routes'].sample(60, 13).items()
    spk, env = speaker_over(world, items, 20)
    healthy = run_test(spk, env, True)
    assert spk._test_sweep[1].fallbacks == 0
    spk, env = speaker_over(world, items, 20)                         # a fresh sweep: its graphs are captured starved
    runtime.take_fault(torch.device('cuda', 0))
    _lib.lib.sf_debug_persist_timeout(0)
    try:
        starved = run_test(spk, env, True)
    finally:
        _lib.lib.sf_debug_persist_timeout(-1)
        torch.cuda.synchronize()
        runtime.take_fault(torch.device('cuda', 0))
    sweep = spk._test_sweep[1]
    assert sweep.fallbacks == 1 and {k[2] for k in sweep.graphs} == {True, False}
    assert {k: v[0] for k, v in starved[0].items()} == {k: v[0] for k, v in healthy[0].items()}       # the words
    assert starved[2] == healthy[2] and np.isfinite(starved[1]).all()
