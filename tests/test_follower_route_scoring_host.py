"""CPU: the host side of the follower's index-form route scoring (Seq2SeqAgent._score_obs_actions_and_instructions on
observations without dense features).

* follower.route_index_batch turns (path_obs, path_actions) into the [S,B] grids of a teacher-forced FollowerEngine pass:
  checked cell by cell against the observation each step of the host loop stands at, with each distinct observation
  dictionary read once, and for the routes the device pass refuses;
* follower.scored_route_outputs builds the host loop's result dictionaries from the pass's [S,B] actions, step scores
  and live flags: checked against a literal restatement of the host loop's bookkeeping (follower.py:342-428), driven by
  a stand-in scorer, with the engine's latched `ended` flag modelled step by step.  Trajectories, actions, per-step
  scores and the float32 running sums must be identical."""
import numpy as np
import pytest

F32 = np.float32


class CountingDict(dict):
    """An observation dictionary that counts how often its candidate list is read."""
    reads = 0

    def __getitem__(self, k):
        if k == 'adj_loc_list':
            CountingDict.reads += 1
        return dict.__getitem__(self, k)


def make_obs(rng, instr_id, enc, n_obs, vp0):
    obs = []
    for t in range(n_obs):
        n_adj = int(rng.integers(2, 7))
        adj = [dict(absViewIndex=-1, rel_heading=0.0, rel_elevation=0.0, nextViewpointId='stop')]
        for a in range(1, n_adj):
            adj.append(dict(absViewIndex=int(rng.integers(0, 36)), rel_heading=float(rng.uniform(-3, 3)),
                            rel_elevation=float(rng.uniform(-0.6, 0.6)), nextViewpointId='v%d' % a))
        view = int(rng.integers(0, 36))
        obs.append(CountingDict(instr_id=instr_id, viewpoint='vp%d' % (vp0 + t), heading=(view % 12) * 0.5236,
                                elevation=(view // 12 - 1) * 0.5236, vp_row=vp0 + t, viewIndex=view,
                                adj_loc_list=adj, instr_encoding=enc))
    return obs


def make_routes(seed=3, late=True):
    """Routes that stop, routes that end without a stop, one-step routes, routes longer than the episode, (late) a
    stop at step 7 of 9; several candidate instructions per route sharing its observation list."""
    rng = np.random.default_rng(seed)
    path_obs, path_actions, instr = [], [], []
    kinds = [('stop', 4), ('open', 3), ('stop', 1), ('open', 1), ('stop', 9), ('open', 8), ('late', 9), ('stop', 2)]
    for r, (kind, m) in enumerate(kinds):
        if kind == 'late' and not late:
            continue
        obs = make_obs(rng, '%d_0' % r, rng.integers(4, 50, size=5), m + 1, 100 * r)
        acts = [int(rng.integers(1, len(obs[t]['adj_loc_list']))) for t in range(m)]
        if kind == 'stop':
            acts[-1] = 0
        elif kind == 'late':                  # a stop behind the last step a 6-step episode runs
            acts[7] = 0
        for c in range(int(rng.integers(1, 5))):          # candidate instructions of ragged lengths
            path_obs.append(obs)
            path_actions.append(acts)
            instr.append(list(rng.integers(4, 90, size=int(rng.integers(1, 30)))))
    return path_obs, path_actions, instr


def score_of(t, b, vp, view, a):
    """Stand-in for the decoder's log-probability of action a: float32 values whose sums depend on the order."""
    return F32(-(0.1 * vp + 0.0137 * view + 0.31 * a + 0.07 * t) / 3.0 - 1e-3 * b - 1.0 / (3.0 + b + t))


def host_loop(path_obs, path_actions, instr, episode_len):
    """follower.py:342-428's bookkeeping, literally (rows walked in instruction-length order like the host loop);
    the decoder replaced by score_of."""
    B = len(path_obs)
    lengths = [len(e) for e in instr]
    perm = list(np.argsort(-np.asarray(lengths), kind='stable'))
    ended = np.array([False] * B)
    sequence_scores = np.zeros(B, F32)
    traj = [{'instr_id': path_o[0]['instr_id'],
             'trajectory': [(path_o[0]['viewpoint'], path_o[0]['heading'], path_o[0]['elevation'])],
             'actions': [], 'scores': [], 'observations': [path_o[0]],
             'instr_encoding': path_o[0]['instr_encoding']} for path_o in path_obs]
    obs = None
    for t in range(episode_len):
        next_obs, next_target_list = [], []
        for perm_index, src_index in enumerate(perm):
            path_o, path_a = path_obs[src_index], path_actions[src_index]
            if t < len(path_a):
                next_target_list.append(path_a[t])
                next_obs.append(path_o[t])
            else:
                next_target_list.append(-1)
                next_obs.append(obs[perm_index])
        obs = next_obs
        target = np.array(next_target_list)
        a_t = np.clip(target, 0, None)
        raw = np.array([score_of(t, perm[i], ob['vp_row'], ob['viewIndex'], a_t[i]) for i, ob in enumerate(obs)], F32)
        action_scores = raw * (target != -1).astype(F32)                  # ignore_index rows score 0
        sequence_scores = sequence_scores + action_scores
        for perm_index, src_index in enumerate(perm):
            ob = obs[perm_index]
            if not ended[perm_index]:
                traj[src_index]['trajectory'].append((ob['viewpoint'], ob['heading'], ob['elevation']))
                traj[src_index]['score'] = float(sequence_scores[perm_index])
                traj[src_index]['scores'].append(float(action_scores[perm_index]))
                traj[src_index]['actions'].append(int(a_t[perm_index]))
        for i in range(B):
            if a_t[i] == 0:
                ended[i] = True
        if ended.all():
            break
    return traj


def engine_model(fb, S):
    """What FollowerEngine leaves in actions / step_scores / live after a teacher-forced pass over the grids: `ended`
    latched (csrc/sf_glue.h), the step score of the action taken whether its target is live or not."""
    B = fb.vp.shape[1]
    ended = np.zeros(B, bool)
    actions, scores, live = np.zeros((S, B), np.int64), np.zeros((S, B), F32), np.zeros((S, B), F32)
    for t in range(S):
        tgt = np.where(ended, -1, fb.target[t])
        actions[t] = np.maximum(tgt, 0)
        scores[t] = [score_of(t, b, fb.vp[t, b], fb.view[t, b], actions[t, b]) for b in range(B)]
        live[t] = tgt >= 0
        ended |= actions[t] == 0
    return actions, scores, live


def f32_sum(xs):
    s = F32(0)
    for x in xs:
        s = F32(s + F32(x))
    return float(s)


@pytest.mark.parametrize('episode_len', [6, 8, 10, 1])
def test_assembled_results_equal_the_host_loop(episode_len):
    from speaker_follower_amd import follower
    path_obs, path_actions, instr = make_routes(late=episode_len <= 8)
    fb, S = follower.route_index_batch(path_obs, path_actions, instr, episode_len)
    got = follower.scored_route_outputs(path_obs, path_actions, *engine_model(fb, S))
    want = host_loop(path_obs, path_actions, instr, episode_len)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w                                     # every list and every float exactly
        assert type(g['score']) is float and all(type(a) is int for a in g['actions'])
    # the quirks, spelled out on the rows that show them
    for g, po, pa in zip(got, path_obs, path_actions):
        assert g['trajectory'][0] == g['trajectory'][1]                    # the first observation twice
        assert g['observations'] == [po[0]]
        if len(pa) < episode_len and pa[-1] != 0:                          # ends without a stop: one more entry
            assert g['actions'] == pa + [0] and g['scores'][-1] == 0.0
            assert g['trajectory'][-1] == g['trajectory'][-2]
            assert g['score'] == f32_sum(g['scores'][:-1])
        assert g['score'] == f32_sum(g['scores'])


def test_grids_follow_the_host_loop_layout():
    from speaker_follower_amd import follower
    from speaker_follower_amd.features import cand_sincos
    path_obs, path_actions, instr = make_routes(seed=8)
    episode_len = 6
    CountingDict.reads = 0
    fb, S = follower.route_index_batch(path_obs, path_actions, instr, episode_len)
    # every distinct observation the pass stands at is read once (the candidates of a route share their observations)
    used = {id(po[min(t, len(pa) - 1)]) for po, pa in zip(path_obs, path_actions) for t in range(S)}
    assert CountingDict.reads == len(used)
    stop_at = [next((t for t, a in enumerate(pa) if a == 0), len(pa)) for pa in path_actions]
    assert S == min(episode_len, max(stop_at) + 1)
    B = len(path_obs)
    A = fb.a_max
    assert A == max(len(dict.__getitem__(po[min(t, len(pa) - 1)], 'adj_loc_list'))
                    for po, pa in zip(path_obs, path_actions) for t in range(S))
    assert fb.vp.shape == fb.view.shape == fb.a_num.shape == fb.target.shape == (S, B)
    assert fb.cand_view.shape == fb.cand_heading.shape == fb.cand_elevation.shape == (S, B, A)
    assert fb.instr == instr
    for b, (po, pa) in enumerate(zip(path_obs, path_actions)):
        for t in range(S):
            ob = po[min(t, len(pa) - 1)]
            adj = dict.__getitem__(ob, 'adj_loc_list')
            assert (fb.vp[t, b], fb.view[t, b], fb.a_num[t, b]) == (ob['vp_row'], ob['viewIndex'], len(adj))
            assert fb.target[t, b] == (pa[t] if t < len(pa) else -1)
            for a in range(1, len(adj)):
                assert fb.cand_view[t, b, a] == adj[a]['absViewIndex']
                assert fb.cand_heading[t, b, a] == adj[a]['rel_heading']            # (float64: no rounding)
                assert fb.cand_elevation[t, b, a] == adj[a]['rel_elevation']
            assert not fb.cand_view[t, b, len(adj):].any() and fb.cand_view[t, b, 0] == 0
    # what the engine's upload computes from them equals the dense path's float64 sin / cos, rounded once
    d = dict.__getitem__(path_obs[0][0], 'adj_loc_list')[1]
    np.testing.assert_array_equal(cand_sincos(fb.cand_heading, fb.cand_elevation)[0, 0, 1],
                                  np.array([np.sin(d['rel_heading']), np.cos(d['rel_heading']),
                                            np.sin(d['rel_elevation']), np.cos(d['rel_elevation'])], F32))


def test_routes_the_device_pass_cannot_reproduce_are_refused():
    from speaker_follower_amd import follower
    path_obs, path_actions, instr = make_routes(seed=4)
    ok = path_actions[0]
    assert ok[-1] == 0 and len(ok) >= 3
    mid = [ok[0], 0] + ok[2:]                                              # a stop before the last action
    with pytest.raises(ValueError, match='stops at step 1'):
        follower.route_index_batch(path_obs[:1], [mid], instr[:1], 10)
    # ... unless the step behind it is never run
    follower.route_index_batch(path_obs[:1], [mid], instr[:1], 2)
    with pytest.raises(ValueError):
        follower.route_index_batch(path_obs[:1], [[]], instr[:1], 10)     # an empty route
    n_adj = len(path_obs[0][0]['adj_loc_list'])
    with pytest.raises(ValueError, match='candidates'):
        follower.route_index_batch(path_obs[:1], [[n_adj] + ok[1:]], instr[:1], 10)
    with pytest.raises(ValueError, match='candidates'):
        follower.route_index_batch(path_obs[:1], [[-2] + ok[1:]], instr[:1], 10)


def test_scores_accumulate_in_float32_step_order():
    """The running score is the float32 sum in step order, not a float64 or pairwise sum."""
    from speaker_follower_amd import follower
    vals = np.array([[1e8], [1.0], [-1e8], [1.0]], F32)                     # float32: 1e8 + 1 == 1e8
    ob = dict(instr_id='0_0', viewpoint='a', heading=0.0, elevation=0.0, instr_encoding=[5])
    out = follower.scored_route_outputs([[ob] * 5], [[1, 1, 1, 1]], np.ones((4, 1), np.int64), vals,
                                        np.ones((4, 1), F32))
    assert out[0]['score'] == 1.0 and out[0]['actions'] == [1, 1, 1, 1]
    assert out[0]['scores'] == [1e8, 1.0, -1e8, 1.0]
    assert len(out[0]['trajectory']) == 5


def test_index_form_call_without_a_feature_store_says_so():
    """Index-form observations on an agent with neither agent.store nor an env-carried store: a clear error, not a
    KeyError on 'feature'."""
    from types import SimpleNamespace
    from speaker_follower_amd import agents
    path_obs, path_actions, instr = make_routes()
    agent = agents.Seq2SeqAgent(SimpleNamespace(), '/dev/null', None, None, episode_len=6)
    with pytest.raises(RuntimeError, match='FeatureStore'):
        agent._score_obs_actions_and_instructions(path_obs, path_actions, instr)
