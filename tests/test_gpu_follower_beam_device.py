"""GPU: the follower's beam search with its step loop on the device (Seq2SeqAgent.beam_on_device,
search.DeviceFollowerBeam, sf_follower_beam_select): the kernel against its numpy model bit for bit, the search against
the reference's outputs (golden G7) and against the host loop (frontier.beam_search) at the rational follower's size,
the loop's own determinism, its host reads, the fallback and the rational follower with the switch on."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import search_world as W                            # noqa: E402
import test_follower_beam_device_host as M          # noqa: E402  (the kernel's numpy model, the synthetic tables)

F32 = np.float32
V = 36
SCORE_TOL = 3e-4                  # test_gpu_search.py: a score is a sum of <= 12 log-probabilities
PATH_TOL = 2e-5                   # test_gpu_search.py: its production and numpy paths at batch 64, K = 40
MAX_EXCUSED = 2                   # of 64 instances (the cap of the same test)


def check_candidates(got, want):
    """tests/test_gpu_search.py: check_candidates, its bounds taken over unchanged."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g['instr_id'] == w['instr_id']
        assert [int(a) for a in g['actions']] == w['actions']
        assert [p[0] for p in g['trajectory']] == w['viewpoints']
        assert abs(g['score'] - w['score']) <= SCORE_TOL * max(1.0, abs(w['score']))
        np.testing.assert_allclose(g['scores'], w['scores'], rtol=2e-4, atol=2e-4)


def make_follower(env, table, seed, episode_len, peaky=False, path='/tmp/sf_fol_beam_dev.json'):
    from speaker_follower_amd import model, features, agents, synth
    d = synth.FULL
    enc_w, dec_w = (synth.follower_weights_peaky if peaky else synth.follower_weights)(seed)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    agent = agents.Seq2SeqAgent(env, path, enc.cuda().eval(), dec.cuda().eval(), episode_len=episode_len)
    agent.store = features.FeatureStore(table)
    return agent


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'g7_search.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def world():
    env, table = W.build_world(dense=True)
    return env, make_follower(env, table, W.FOLLOWER_SEED, W.EPISODE_LEN)


class switched_on:
    def __init__(self, agent, **kw):
        self.agent, self.kw = agent, dict(kw, beam_on_device=True)

    def __enter__(self):
        for k, v in self.kw.items():
            setattr(self.agent, k, v)
        return self.agent

    def __exit__(self, *exc):
        for k in self.kw:
            delattr(self.agent, k)                  # (back to the class defaults)
        return False


def copy_hist(db):
    return {k: np.array(v, copy=True) for k, v in db.last.items()}


def assert_hist_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (what, k)


# ----------------------------------------------------------------------------------------------- 4. kernel alone
@pytest.mark.parametrize('B,beam', [(1, 1), (1, 3), (64, 3), (1, 40), (64, 40), (1, 64), (64, 64)])
def test_select_kernel_equals_its_numpy_model_bit_for_bit(B, beam):
    """sf_follower_beam_select alone over E + 1 launches on synthetic tables: exact score ties, lists that end at a
    -1 or at an action the state does not have, states with fewer than k candidates, instances that finish at
    different steps.  Exact, because the only arithmetic is one float32 add."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd._lib import call
    from speaker_follower_amd.runtime import ptr, stream
    rng = np.random.default_rng(1000 * B + beam)
    E, T = 7, 12
    nav, A = M.synthetic_nav(beam + B, n_rows=11, A=8)
    k, R = min(beam, A), B * beam
    dev = torch.device('cuda')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)              # noqa: E731
    d_nav = {n: up(nav[n]) for n in ('a_num', 'next_row', 'cand_view', 'sincos', 'feat_row')}
    nav_s = _lib.NavTableS(*(d_nav[n].data_ptr() for n in ('a_num', 'next_row', 'cand_view', 'sincos', 'feat_row')), A, V)
    s = M.new_state(B, beam, E, T, rng.integers(0, 11 * V, B))
    names = ('score', 'row', 'view', 'act', 'parent', 'inst', 'live_total', 'hist_parent', 'hist_action', 'hist_rank',
             'hist_sid', 'hist_psid', 'hist_score', 'hist_attn', 'done_rec', 'done_score')
    # the history arrays of one step are R apart inside one buffer, as DeviceFollowerBeam lays them out
    S = R * (6 + T)
    rec = torch.zeros(E * S, dtype=torch.int32, device=dev)
    rec.view(E, S)[:, R:2 * R].fill_(-1)
    d = {n: up(s[n]) for n in names if not n.startswith('hist_')}
    p0 = rec.data_ptr()
    fb = _lib.FolBeam(B, beam, k, E, T, 0, nav_s, d['score'].data_ptr(), d['row'].data_ptr(), d['view'].data_ptr(),
                      d['act'].data_ptr(), d['parent'].data_ptr(), d['inst'].data_ptr(), d['live_total'].data_ptr(),
                      *(p0 + 4 * j * R for j in range(7)), S, d['done_rec'].data_ptr(), d['done_score'].data_ptr())
    for step in range(E + 1):
        top_a = rng.integers(0, A, (R, k)).astype(np.int32)                       # dead slots: junk that must be ignored
        top_lp = rng.standard_normal((R, k)).astype(F32)
        alpha = rng.random((R, T)).astype(F32)
        for b in range(B):
            for i in range(int(s['inst'][b, 0])):
                r = b * beam + i
                sid = int(s['row'][r]) * V + int(s['view'][r])
                lp = (-0.5 * rng.integers(0, 4, A)).astype(F32)                   # coarse: exact ties after the add
                if rng.random() < 0.3:
                    lp = (lp + rng.standard_normal(A).astype(F32) * F32(0.37)).astype(F32)
                lp[0] = F32(-0.5 * rng.integers(0, 3)) if step >= 1 + b % 3 else F32(-9.0)
                # mostly what sf_logprob_topk(n_valid = a_num) gives; sometimes the whole row, so that an action the
                # state does not have stands in the middle of the list and ends it
                n_valid = A if rng.random() < 0.2 else int(nav['a_num'][sid])
                top_a[r], top_lp[r] = M.topk_valid(lp, n_valid, k)
        M.model_step(s, nav, top_a, top_lp, alpha)
        d_a, d_lp, d_alpha = up(top_a), up(top_lp), up(alpha)
        call('sf_follower_beam_select', C.byref(fb), ptr(d_a), ptr(d_lp), ptr(d_alpha), stream())
        torch.cuda.synchronize()
        got = rec.cpu().numpy().reshape(E, S)
        for j, n in enumerate(('hist_parent', 'hist_action', 'hist_rank', 'hist_sid', 'hist_psid')):
            assert np.array_equal(got[:, j * R:(j + 1) * R], s[n]), (step, n)
        assert np.array_equal(got[:, 5 * R:6 * R], s['hist_score'].view(np.int32)), (step, 'hist_score')
        assert np.array_equal(got[:, 6 * R:].reshape(E, R, T), s['hist_attn'].view(np.int32)), (step, 'hist_attn')
        for n in names:
            if not n.startswith('hist_'):
                assert np.array_equal(d[n].cpu().numpy().view(np.int32), s[n].view(np.int32)), (step, n)
    assert (s['inst'][:, 2] <= E).all() and (s['inst'][:, 0] == 0).all()
    assert s['inst'][:, 1].max() == 2 * beam - 1 or beam < 3 or B == 1      # (the completion list's last place was used)
    if B > 1:
        assert len(set(s['inst'][:, 2].tolist())) > 1, 'every instance ended at the same step'
    sc = s['hist_score'][s['hist_action'] >= 0]
    assert beam == 1 or len(np.unique(sc)) < len(sc), 'no exact ties among the selections'


# ------------------------------------------------------------------------------------------------ 5. the reference
@pytest.mark.parametrize('beam', [1, 3, 5])
def test_device_beam_search_matches_reference(world, golden, beam):
    env, agent = world
    env.set_beam_size(beam)
    env.reset_epoch()
    got = []
    with switched_on(agent):
        before = agent.beam_fallbacks
        for _ in range(W.N_ITEMS // W.BATCH):
            trajs, completed, traversed = agent.beam_search(beam)
            assert traversed is None and len(completed) == len(trajs)
            got += trajs
        assert agent.beam_fallbacks == before == 0
        db = agent.device_beam
        assert db is not None and db.graph is not None and db.minibatches >= 2 and db.beam == beam
    want = golden['beam'][str(beam)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        check_candidates(g, w)
    for tl in got:
        for c in tl:
            assert len(c['attentions']) == len(c['actions'])
            np.testing.assert_allclose([a.sum() for a in c['attentions']], 1.0, rtol=1e-5)
    for hyps, tl in zip(completed, trajs):                 # the hypothesis views of the completions
        for h in hyps:
            assert h.world_state.scanId and h.observation['viewpoint'] == h.world_state.viewpointId
            assert h.action_count >= 1 and h.prev_inference_state is not None
            assert h.last_action == 0 or h.action_count == W.EPISODE_LEN
        assert sorted(c['score'] for c in tl) == sorted(h.score for h in hyps)[-len(tl):]


def test_device_beam_one_equals_greedy_rollout(world):
    """tests/test_gpu_search.py::test_beam_one_equals_greedy_rollout with the switch on."""
    env, agent = world
    env.set_beam_size(1)
    env.reset_epoch()
    agent.feedback = 'argmax'
    with torch.no_grad():
        greedy = agent._rollout_with_loss()
    with switched_on(agent):
        beams, _, _ = agent.beam_search(1, load_next_minibatch=False)
        assert agent.beam_fallbacks == 0 and agent.device_beam.beam == 1
    assert len(beams) == len(greedy)
    for b, g in zip(beams, greedy):
        assert b[0]['instr_id'] == g['instr_id']
        assert b[0]['trajectory'] == g['trajectory']
        assert abs(b[0]['score'] - g['score']) < 2e-4 * max(1.0, abs(g['score']))


# --------------------------------------------------------------------------------------- 6. the host loop, at size
def _near_tie_instances(log, n_inst, bound):
    """Instances whose host loop cut its successors, or ranked its completions, across a gap <= bound."""
    hit = np.zeros(n_inst, bool)
    for rec in log:
        if rec[0] == 'select':
            hit[rec[2][rec[3] <= bound]] = True
        elif (rec[2] <= bound).any():
            hit[rec[1]] = True
    return hit


def _differing(a, b):
    """Instances whose completions differ (other routes, other order, or a score further apart than PATH_TOL)."""
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        same = len(x) == len(y) and all(
            p['actions'] == q['actions'] and p['trajectory'] == q['trajectory'] and abs(p['score'] - q['score']) <= PATH_TOL
            for p, q in zip(x, y))
        if not same:
            out.append(i)
    return out


def test_device_loop_matches_the_host_loop_at_batch64_beam40():
    """The 64-instruction "peaky" world of test_state_factored_search_batch64_k40_matches_reference, beam 40: the device
    loop gives the host loop's completions in the host loop's order with scores within 2e-5.  The two pad instructions
    and candidate columns differently, so an instance may be excused -- at most 2 of 64 -- only where the host loop's
    own margin log shows a selection or ranking gap at or below that bound.  The cap is first confirmed on the host loop
    against itself under the strict gate products (another summation order): that pair alone stays within it with
    item seed W.BIG_ITEM_SEED = 15."""
    from speaker_follower_amd import runtime
    env, table = W.build_world(dense=True, n_items=W.BIG_ITEMS, batch=W.BIG_BATCH, item_seed=W.BIG_ITEM_SEED)
    agent = make_follower(env, table, W.BIG_FOLLOWER_SEED, W.BIG_EPISODE_LEN, peaky=True)
    beam = W.BIG_K
    env.set_beam_size(beam)
    env.reset_epoch()
    agent.tie_log = []
    host, host_done, _ = agent.beam_search(beam)
    near = _near_tie_instances(agent.tie_log, 64, PATH_TOL)
    del agent.tie_log
    assert len(host) == 64 and sum(len(x) for x in host) > 64 * 20
    with runtime.strict_gate_product():
        env.reset_epoch()
        strict, _, _ = agent.beam_search(beam)
    d_strict = _differing(strict, host)
    print('host loop against itself under strict gate products: instances that differ %s; near ties (<= %.0e) in the '
          'host loop\'s margin log: %s' % (d_strict, PATH_TOL, np.flatnonzero(near).tolist()))
    assert all(near[i] for i in d_strict), d_strict
    assert len(d_strict) <= MAX_EXCUSED, d_strict
    env.reset_epoch()
    with switched_on(agent):
        dev, dev_done, _ = agent.beam_search(beam)
        assert agent.beam_fallbacks == 0 and agent.device_beam.graph is not None
        assert agent.device_beam.R == 64 * beam
    d_dev = _differing(dev, host)
    worst = max((abs(p['score'] - q['score']) for i, (x, y) in enumerate(zip(dev, host)) if i not in d_dev
                 for p, q in zip(x, y)), default=0.0)
    print('device loop against the host loop: instances that differ %s; worst score difference elsewhere %.2e'
          % (d_dev, worst))
    assert all(near[i] for i in d_dev), [i for i in d_dev if not near[i]]
    assert len(d_dev) <= MAX_EXCUSED, d_dev
    for i, (hd, hh) in enumerate(zip(dev_done, host_done)):
        if i not in d_dev:
            assert len(hd) == len(hh)


# ------------------------------------------------------------------------------ 7. / 8. the loop itself, host reads
@pytest.fixture(scope='module')
def mid():
    """24 instructions in minibatches of 12 on the fixture graphs, peaky weights, 7 steps."""
    env, table = W.build_world(dense=True, n_items=24, batch=12, item_seed=9)
    agent = make_follower(env, table, 77, 7, peaky=True)
    env.set_beam_size(6)
    return env, agent


def _two_minibatches(env, agent, beam, chunk, graphs, fresh=False):
    """The first two minibatches of the epoch through the device loop: [(history, results, DeviceFollowerBeam)].
    fresh: each on a newly built DeviceFollowerBeam instead of the agent's cached one."""
    from speaker_follower_amd import search
    out = []
    env.reset_epoch()
    for _ in range(2):
        if fresh:
            agent.__dict__.pop('_device_beams', None)
        res = search.beam_search_device(agent, beam, chunk=chunk, graphs=graphs)
        db = agent.device_beam
        assert db.chunk == chunk and db.graphs == graphs
        assert db.last_host_reads <= math.ceil(agent.episode_len / chunk) + 1, (chunk, db.last_host_reads)
        out.append((copy_hist(db), res, db))
    return out


def test_replay_equals_eager_issue_and_every_chunk_size_gives_the_same_history(mid):
    env, agent = mid
    E, beam = agent.episode_len, 6
    ref = None
    for chunk, graphs in ((3, True), (1, True), (E, True), (3, False), (1, False), (E, False)):
        runs = _two_minibatches(env, agent, beam, chunk, graphs)
        db = runs[0][2]
        assert runs[1][2] is db and (db.graph is not None) == graphs and db.captures == (1 if graphs else 0)
        print('chunk %d, graphs %s: host reads %s of at most %d' % (chunk, graphs, db.last_host_reads,
                                                                   math.ceil(E / chunk) + 1))
        if ref is None:
            ref = runs
            continue
        for m in range(2):
            assert_hist_equal(runs[m][0], ref[m][0], (chunk, graphs, m))
    assert (ref[0][0]['inst'][:, 1] >= 1).all() and ref[0][0]['action'].shape[0] >= 2


def test_no_state_leaks_between_searches_through_the_same_graph(mid):
    """Two consecutive minibatches through one captured graph equal the same two minibatches run each on a freshly
    built DeviceFollowerBeam; and a search repeated on the same object gives the same history."""
    env, agent = mid
    agent.__dict__.pop('_device_beams', None)
    shared = _two_minibatches(env, agent, 6, 3, True)
    assert shared[0][2] is shared[1][2] and shared[0][2].captures == 1
    fresh = _two_minibatches(env, agent, 6, 3, True, fresh=True)
    assert fresh[0][2] is not fresh[1][2] and fresh[0][2] is not shared[0][2]
    for m in range(2):
        assert_hist_equal(shared[m][0], fresh[m][0], m)
    assert not np.array_equal(shared[0][0]['sid'], shared[1][0]['sid'])     # (two different minibatches)
    again = _two_minibatches(env, agent, 6, 3, True)
    for m in range(2):
        assert_hist_equal(again[m][0], fresh[m][0], ('again', m))


def test_a_moved_weight_recaptures_the_graph(mid):
    from speaker_follower_amd import search
    env, agent = mid
    agent.__dict__.pop('_device_beams', None)
    env.reset_epoch()
    search.beam_search_device(agent, 6, chunk=3, graphs=True)
    db = agent.device_beam
    first = copy_hist(db)
    assert db.captures == 1
    p = agent.decoder.lstm.bias_ih
    old = p.data
    try:
        p.data = (old * 1.5 + 0.01).clone()                 # an update that puts the weight somewhere else
        env.reset_epoch()
        search.beam_search_device(agent, 6, chunk=3, graphs=True)
        assert agent.device_beam is db and db.captures == 2
        moved = copy_hist(db)
        env.reset_epoch()
        search.beam_search_device(agent, 6, chunk=3, graphs=False)
        assert agent.device_beam is not db and agent.device_beam.graph is None
        assert_hist_equal(moved, copy_hist(agent.device_beam), 'after the update')
        assert not np.array_equal(moved['score'], first['score'])
    finally:
        p.data = old
    env.reset_epoch()
    search.beam_search_device(agent, 6, chunk=3, graphs=True)
    assert db.captures == 3
    assert_hist_equal(copy_hist(db), first, 'weights restored')


# --------------------------------------------------------------------------------------------------- 9. fallback
def test_wide_beam_falls_back_to_the_host_loop(world):
    env, agent = world
    env.set_beam_size(65)
    env.reset_epoch()
    want, _, _ = agent.beam_search(65)
    env.reset_epoch()
    with switched_on(agent, beam_fallbacks=0, device_beam=None):
        got, _, _ = agent.beam_search(65)
        assert agent.beam_fallbacks == 1 and agent.device_beam is None
    assert len(got) == len(want)
    for gl, wl in zip(got, want):
        assert len(gl) == len(wl)
        for g, w in zip(gl, wl):
            for key in ('instr_id', 'actions', 'score', 'scores', 'trajectory'):
                assert g[key] == w[key], key
            assert all(np.array_equal(x, y) for x, y in zip(g['attentions'], w['attentions']))


# ----------------------------------------------------------------------------------------- 10. rational follower
def test_rational_follower_with_the_switch_on_equals_the_switch_off(world):
    from speaker_follower_amd import model, agents, synth, search
    env, agent = world
    d = synth.FULL
    senc_w, sdec_w = synth.speaker_weights(W.SPEAKER_SEED)
    senc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
    sdec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=sdec_w['embedding.weight'])
    senc.load_state_dict({k: torch.tensor(v) for k, v in senc_w.items()})
    sdec.load_state_dict({k: torch.tensor(v) for k, v in sdec_w.items()})
    speaker = agents.Seq2SeqSpeaker(env, '/tmp/sf_fol_beam_dev_spk.json', senc.cuda().eval(), sdec.cuda().eval(),
                                    W.INSTRUCTION_LEN, max_episode_len=W.EPISODE_LEN)
    off, counts_off = search.run_rational_follower(env, None, agent, speaker, beam_size=3)
    with switched_on(agent, beam_fallbacks=0):
        on, counts_on = search.run_rational_follower(env, None, agent, speaker, beam_size=3)
        assert agent.beam_fallbacks == 0 and agent.device_beam.minibatches >= W.N_ITEMS // W.BATCH
    assert set(on) == set(off) == {0.0, 0.95}
    for w in off:
        assert set(on[w]) == set(off[w]) and len(on[w]) == W.N_ITEMS
        assert counts_on[w] == counts_off[w]
        for instr_id, c in off[w].items():
            g = on[w][instr_id]
            assert [int(a) for a in g['actions']] == [int(a) for a in c['actions']]
            assert g['trajectory'] == c['trajectory']
            assert abs(g['score'] - c['score']) <= SCORE_TOL * max(1.0, abs(c['score']))
            np.testing.assert_allclose(g['scores'], c['scores'], rtol=2e-4, atol=2e-4)
            assert abs(g['speaker_score'] - c['speaker_score']) <= SCORE_TOL * max(1.0, abs(c['speaker_score']))
