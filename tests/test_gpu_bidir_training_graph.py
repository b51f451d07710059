"""GPU: whole training iterations with a BIDIRECTIONAL encoder (train.py --bidirectional) as hipGraph replays
(FollowerEngine.capture_training, runtime.TrainingGraph): the encoder's forward and backward are the C entries
sf_encoder_bilstm_fwd / _bwd on the engine's fixed tapes, so the iteration is capturable; replays equal the eager loop.
And Seq2SeqAgent.train takes the replayed iterations for such an encoder (single process)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import search_world as W                                              # noqa: E402
from speaker_follower_amd import synth                                # noqa: E402

EPISODE = 7


def _bidir_follower(enc_seed=19, dec_seed=21):
    from speaker_follower_amd import model
    d = synth.FULL
    w = synth.bidirectional_encoder_weights(enc_seed)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden // 2, 0, 0.5, bidirectional=True, glove=w['embedding.weight'])
    enc.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    _, dec_w = synth.follower_weights_peaky(dec_seed)
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    return enc.cuda().train(), dec.cuda().train()


def _weights(mods):
    return torch.cat([p.detach().reshape(-1) for m in mods for p in m.parameters()]).clone()


@pytest.mark.parametrize('feedback', ['teacher', 'sample'])
def test_bidirectional_training_graph_equals_the_eager_loop(feedback):
    from speaker_follower_amd import features, follower as fol, optim
    B, S, NVP, N = 48, 6, 96, 5
    fb = synth.follower_batch(seed=3, batch=B, steps=S, n_viewpoints=NVP, min_len=8, max_len=40)
    store = features.FeatureStore(synth.feature_table(3, NVP))
    batch = fol.DeviceFollowerBatch.from_synth(fb)
    out = {}
    for mode in ('eager', 'graph'):
        enc, dec = _bidir_follower()
        oe = optim.FusedAdam([p for p in enc.parameters() if p.requires_grad], lr=1e-3, weight_decay=5e-4)
        od = optim.FusedAdam([p for p in dec.parameters() if p.requires_grad], lr=1e-3, weight_decay=5e-4)
        eng = fol.FollowerEngine(enc, dec, store)
        eng.dropout_seed = 777
        eng.two_stream_backward = False                            # (one stream: bit-equal weights)
        losses, acts, sites = [], [], []
        if mode == 'eager':
            for _ in range(N):
                oe.zero_grad()
                od.zero_grad()
                st = eng.rollout(batch, S, feedback, train=True)
                st.loss.backward()
                oe.step()
                od.step()
                losses.append(float(st.loss.detach()))
                acts.append(st.actions.cpu().numpy().copy())
                sites.append(st.site0)
        else:
            tg = eng.capture_training(batch, S, feedback, optimizers=(oe, od))      # (runs iteration 1 eagerly)
            losses.append(float(tg.first.loss_buf))
            acts.append(tg.first.actions.cpu().numpy().copy())
            sites.append(tg.first.site0)
            for _ in range(N - 1):
                st = tg.replay()
                torch.cuda.synchronize()
                losses.append(float(st.loss_buf))
                acts.append(st.actions.cpu().numpy().copy())
                sites.append(st.site0)
            assert tg.replays == N - 1 and eng.iteration == N
        torch.cuda.synchronize()
        assert enc.last_path == enc.last_backward_path == 'persistent'
        out[mode] = (losses, acts, sites, _weights((enc, dec)), oe.host_steps() + od.host_steps())
    le, lg = out['eager'][0], out['graph'][0]
    print('[bidir training graph, %s] losses eager %s | graph %s' % (feedback, ['%.5f' % x for x in le],
                                                                     ['%.5f' % x for x in lg]))
    assert out['eager'][2] == out['graph'][2]                      # the same sites ...
    assert out['eager'][4] == out['graph'][4] == [N, N]            # ... and Adam steps
    assert len(set(le)) == N
    for a, b in zip(out['eager'][1], out['graph'][1]):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(lg, le, rtol=2e-6)
    assert torch.equal(out['eager'][3], out['graph'][3])


@pytest.fixture(scope='module')
def world():
    from speaker_follower_amd import features, nav
    env, table = W.build_world(dense=True, n_items=24, batch=12, item_seed=77)
    store = features.FeatureStore(table)
    return env, store, nav.NavTable(env, store)


def _agent(world, graph):
    from speaker_follower_amd import agents, optim
    env, store, nt = world
    enc, dec = _bidir_follower(23, 303)
    torch.manual_seed(4)
    ag = agents.Seq2SeqAgent(env, '/tmp/sf_bidir_train.json', enc, dec, episode_len=EPISODE)
    ag.store = store
    ag.use_device_env(nt)
    ag.train_graph = graph
    oe = optim.FusedAdam([p for p in enc.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)
    od = optim.FusedAdam([p for p in dec.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)
    import random
    if not hasattr(env, '_items_in_order'):
        env._items_in_order = list(env.data)
    env.data[:] = env._items_in_order
    random.seed(11)
    env.reset_epoch()
    return ag, oe, od, lambda: _weights((enc, dec))


def test_agent_trains_a_bidirectional_encoder_on_graph_replays(world):
    out = {}
    for graph in (False, True):
        ag, oe, od, weights = _agent(world, graph)
        ag.feedback = 'teacher'
        assert ag._graph_trainable(oe, od) == graph
        ag.train(oe, od, 4, feedback='teacher')
        assert (ag.__dict__.get('_train_graph_state') is not None) == graph
        if graph:
            assert ag._train_graph_state[1].replays == 3 and oe.host_steps() == [4] and od.host_steps() == [4]
        out[graph] = (list(ag.losses), weights())
    print('[bidir agent.train] losses eager', out[False][0], 'graph', out[True][0])
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=2e-4)
    assert len(set(out[True][0])) == 4
    d = (out[True][1] - out[False][1]).abs().max().item()
    print('[bidir agent.train] max weight difference graph vs eager after 4 iterations: %.2e' % d)
    assert d < 3e-4 and torch.isfinite(out[True][1]).all()
