"""GPU: the agent-level re-issues after a persistent-launch fault that no other test walks -- an inference rollout on a
replayed graph, a chunked route-scoring call, the eager training loops of the follower and of the speaker, the
speaker's index-route training iteration.  Nothing is made to fault: the fault word is raised from the host
(`runtime.fault_word(device).fill_(...)`) at the moment a starved launch would have raised it, by wrapping one Python
callable of one instance for its first call.  Every test compares against an undisturbed twin built with the same
seeds."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import search_world as W                                                           # noqa: E402
from speaker_follower_amd import synth                                             # noqa: E402
from tests.test_gpu_nav import world, _fresh_agent                                 # noqa: E402,F401
from tests.test_gpu_follower_route_scoring import routes, candidate_rows           # noqa: E402,F401

DEV = torch.device('cuda', 0)


def raise_after_first_call(fn, bit):
    """`fn`, raising `bit` in the current stream's fault word behind its FIRST call (as if a persistent launch issued
    by that call -- or by the backward that follows it -- had starved)."""
    from speaker_follower_amd import runtime
    calls = []

    def wrapped(*a, **k):
        calls.append(1)
        out = fn(*a, **k)
        if len(calls) == 1:
            runtime.fault_word(DEV).fill_(bit)
        return out
    return wrapped


def recording(fn, seen):
    def wrapped(*a, **k):
        seen.append(fn(*a, **k))
        return seen[-1]
    return wrapped


def test_a_fault_under_a_replayed_inference_rollout_is_repaired_eagerly(world):
    """Seq2SeqAgent._rollout_on_graph: the fault word raised behind the first replay of a test() call."""
    from speaker_follower_amd import runtime
    out = {}
    for poison in (False, True):
        ag, oe, od, weights = _fresh_agent(world, False)
        ag.test(use_dropout=False, feedback='argmax')          # (healthy: captures the graph)
        (key, cached), = ag._test_graphs.items()
        inflight = []
        on_graph = ag._rollout_on_graph

        def watched(*a, **k):
            res = on_graph(*a, **k)
            inflight.append('_rollout_inflight' in ag.__dict__)
            return res
        ag._rollout_on_graph = watched
        if poison:
            ag._test_graphs[key] = (raise_after_first_call(cached[0], runtime.FAULT_ENC_FWD),) + cached[1:]
        try:
            res = ag.test(use_dropout=False, feedback='argmax')
        finally:
            del ag._rollout_on_graph
            ag._test_graphs[key] = cached
        out[poison] = (res, list(ag.losses), ag._engine.fallbacks, inflight)
        assert getattr(ag.encoder, 'persistent', True) is True
    a, b = out[True][0], out[False][0]
    assert sorted(a) == sorted(b) and len(a) > 0
    for k in a:
        assert a[k]['actions'] == b[k]['actions'] and a[k]['trajectory'] == b[k]['trajectory']
    print('[site 5] losses repaired', out[True][1], 'undisturbed', out[False][1])
    assert out[True][2] == 1 and out[False][2] == 0
    assert out[False][3][0] is True and out[True][3][0] is False   # (what was issued ahead is dropped by the repair)


def test_a_fault_under_a_chunked_route_scoring_call_reissues_every_chunk(routes):
    """Seq2SeqAgent._score_routes_on_device: the call does not clear the fault words on entry, so a word raised just
    before it is what a starved launch of its first chunk would leave."""
    from speaker_follower_amd import runtime
    follower, variants = routes
    _, index, acts, instr = candidate_rows(variants, 40)
    follower.SCORE_CHUNK = 16                                   # (3 chunks)
    try:
        with torch.no_grad():
            want, loss_want = follower._score_obs_actions_and_instructions(index, acts, instr)
            assert follower.last_host_reads == 1
            eng = follower._score_engine
            assert eng.fallbacks == 0
            runtime.fault_word(DEV).fill_(runtime.FAULT_ENC_FWD)
            got, loss_got = follower._score_obs_actions_and_instructions(index, acts, instr)
    finally:
        del follower.SCORE_CHUNK
    assert follower.last_host_reads == 3 and eng.fallbacks == 1
    assert getattr(follower.encoder, 'persistent', True) is True
    assert len(got) == len(want) == 40
    for g, w in zip(got, want):
        assert g['actions'] == w['actions'] and g['trajectory'] == w['trajectory']
        np.testing.assert_allclose(g['scores'], w['scores'], rtol=1e-4, atol=2e-4)
    print('[site 6] loss re-issued %.7f undisturbed %.7f' % (float(loss_got), float(loss_want)))
    np.testing.assert_allclose(float(loss_got), float(loss_want), rtol=1e-4, atol=2e-4)


def test_a_fault_under_the_followers_eager_backward_retrains_the_minibatch(world):
    """Seq2SeqAgent.train, launch by launch on the device environment: the fault word raised behind the first rollout
    (seen after its backward) -- the same minibatch again on the per-step kernels, one optimizer step per iteration."""
    from speaker_follower_amd import runtime
    out = {}
    for poison in (False, True):
        ag, oe, od, weights = _fresh_agent(world, False)
        w0 = weights()
        if poison:
            ag._rollout_with_loss = raise_after_first_call(ag._rollout_with_loss, runtime.FAULT_ENC_BWD)
        try:
            ag.train(oe, od, 2, feedback='teacher')
        finally:
            ag.__dict__.pop('_rollout_with_loss', None)
        out[poison] = (list(ag.losses), ag._engine.fallbacks)
        assert len(ag.losses) == 2 and np.isfinite(ag.losses).all()
        assert oe.host_steps() == [2] and od.host_steps() == [2]
        w1 = weights()
        assert torch.isfinite(w1).all() and not torch.equal(w1, w0)
        assert getattr(ag.encoder, 'persistent', True) is True
    print('[site 7] losses re-issued', out[True][0], 'undisturbed', out[False][0], 'fallbacks', out[True][1])
    np.testing.assert_allclose(out[True][0][0], out[False][0][0], rtol=1e-4)
    assert out[True][1] == 1 and out[False][1] == 0


def _speaker_agents(fast):
    """The set-up of test_gpu_agents.py::test_speaker_train_without_outputs_is_the_same_training, twice: an undisturbed
    agent and the one whose fault word is raised."""
    from speaker_follower_amd import agents, features, model, optim, speaker
    env, table = W.build_world(dense=False, n_items=60, batch=12, item_seed=7)
    store = features.FeatureStore(table)
    d = synth.FULL
    w_enc, w_dec = synth.speaker_weights(W.SPEAKER_SEED)
    for poison in (False, True):
        senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
        sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=w_dec['embedding.weight'])
        senc.load_state_dict({k: torch.tensor(v) for k, v in w_enc.items()})
        sdec.load_state_dict({k: torch.tensor(v) for k, v in w_dec.items()})
        senc.cuda()
        sdec.cuda()
        torch.manual_seed(3)
        spk = agents.Seq2SeqSpeaker(env, '/tmp/sf_spk_fault.json', senc, sdec, W.INSTRUCTION_LEN,
                                    max_episode_len=W.EPISODE_LEN)
        spk.store = store
        spk.train_without_outputs = fast
        spk._engine = speaker.SpeakerEngine(senc, sdec, store)
        oe = optim.FusedAdam([p for p in senc.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)
        od = optim.FusedAdam([p for p in sdec.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)
        env.reset_epoch()
        yield poison, spk, oe, od, lambda: torch.cat([p.detach().reshape(-1) for m in (senc, sdec)
                                                      for p in m.parameters()]).clone()


def test_a_fault_under_the_speakers_index_route_iteration_retrains_the_minibatch():
    """Seq2SeqSpeaker._train_iteration_on_index_routes: the fault word raised behind the first scoring pass (seen after
    its backward) -- the same minibatch at the same dropout sites on the per-step kernels."""
    from speaker_follower_amd import runtime
    rng_state = random.getstate()
    out = {}
    try:
        for poison, spk, oe, od, weights in _speaker_agents(True):
            eng, w0, returned = spk._engine, weights(), []
            spk._train_iteration_on_index_routes = recording(spk._train_iteration_on_index_routes, returned)
            if poison:
                eng.score = raise_after_first_call(eng.score, runtime.FAULT_SPEAKER)
            try:
                spk.train(oe, od, 2, feedback='teacher')
            finally:
                eng.__dict__.pop('score', None)
                del spk._train_iteration_on_index_routes
            assert spk._engine is eng and returned == [True, True]
            out[poison] = (list(spk.losses), eng.fallbacks)
            assert len(spk.losses) == 2 and np.isfinite(spk.losses).all()
            assert oe.host_steps() == [2] and od.host_steps() == [2]
            w1 = weights()
            assert torch.isfinite(w1).all() and not torch.equal(w1, w0)
            assert eng.persistent is True
    finally:
        random.setstate(rng_state)
    print('[site 11] losses re-issued', out[True][0], 'undisturbed', out[False][0])
    np.testing.assert_allclose(out[True][0][0], out[False][0][0], rtol=1e-4)
    assert out[True][1] == 1 and out[False][1] == 0


def test_a_fault_under_the_speakers_eager_backward_trains_on_the_next_minibatch():
    """Seq2SeqSpeaker.train with rollout() + loss.backward(): the fault word raised behind the first rollout (seen after
    its backward) -- the iteration is trained on the next minibatch with the per-step kernels."""
    from speaker_follower_amd import runtime
    rng_state = random.getstate()
    try:
        for poison, spk, oe, od, weights in _speaker_agents(False):
            eng, w0 = spk._engine, weights()
            if poison:
                spk.rollout = raise_after_first_call(spk.rollout, runtime.FAULT_SPEAKER)
            try:
                spk.train(oe, od, 2, feedback='teacher')
            finally:
                spk.__dict__.pop('rollout', None)
            print('[site 12] poisoned %s losses' % poison, spk.losses)
            assert spk._engine is eng
            assert len(spk.losses) == 2 and np.isfinite(spk.losses).all()
            assert oe.host_steps() == [2] and od.host_steps() == [2]
            w1 = weights()
            assert torch.isfinite(w1).all() and not torch.equal(w1, w0)
            assert eng.fallbacks == (1 if poison else 0) and eng.persistent is True
    finally:
        random.setstate(rng_state)
