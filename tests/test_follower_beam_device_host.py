"""CPU: the host side of the follower's device beam search (search.DeviceFollowerBeam / sf_follower_beam_select).

* frontier.beam_outputs -- the result assembly the host and device step loops share -- gives what the host loop's own
  tail gave before it was factored out, on a synthetic hypothesis table with exact score ties;
* the device loop's history layout (include/sf_hip.h: sf_follower_beam_select), produced by a step-by-step numpy model
  of the kernel (`model_step`, which tests/test_gpu_follower_beam_device.py holds the kernel to bit for bit) and read
  back through frontier.hypotheses_from_history, gives the host loop's hypothesis table node for node
  (frontier.beam_search over a stand-in decoder whose log-probabilities are a function of the state history, with
  many exact float32 ties and states with fewer than k candidates);
* the margin log of the host loop records what it says and changes nothing;
* the new C entry rejects bad arguments before touching the device."""
import ctypes as C
import zlib

import numpy as np
import pytest

F32 = np.float32
V = 36


# ------------------------------------------------------------------------------------------ the kernel's model
def new_state(B, beam, E, T, root_sid, with_attn=True):
    """The buffers of sf_fol_beam as DeviceFollowerBeam.run presets them."""
    R = B * beam
    sid = np.repeat(np.asarray(root_sid, np.int64), beam)
    s = dict(B=B, beam=beam, E=E, T=T,
             score=np.zeros(R, F32), row=np.tile(sid // V, 2).astype(np.int32), view=np.tile(sid % V, 2).astype(np.int32),
             act=np.zeros(R, np.int32), parent=np.full(R, -1, np.int32), inst=np.zeros((B, 3), np.int32),
             live_total=np.zeros(E, np.int32), done_rec=np.zeros((B, 2 * beam), np.int32),
             done_score=np.zeros((B, 2 * beam), F32))
    s['parent'][::beam] = np.arange(0, R, beam)
    s['inst'][:, 0] = 1
    for name in ('parent', 'action', 'rank', 'sid', 'psid'):
        s['hist_' + name] = np.zeros((E, R), np.int32)
    s['hist_action'][:] = -1
    s['hist_score'] = np.zeros((E, R), F32)
    s['hist_attn'] = np.zeros((E, R, T), F32) if with_attn else None
    return s


def model_step(s, nav, top_a, top_lp, alpha):
    """One launch of sf_follower_beam_select (include/sf_hip.h) on the buffers `s`, in place.  nav: host tables a_num
    [n], next_row / cand_view [n, A]; top_a int32 / top_lp float32 [R, k]; alpha [R, T] or None."""
    B, W, E = s['B'], s['beam'], s['E']
    R, k = B * W, top_a.shape[1]
    for b in range(B):
        live, n_done, t = (int(x) for x in s['inst'][b])
        if live <= 0 or t >= E:
            continue
        base = b * W
        sid_of = [int(s['row'][base + i]) * V + int(s['view'][base + i]) for i in range(live)]
        cands = []
        for i in range(live):
            for j in range(k):
                a = int(top_a[base + i, j])
                if a < 0 or a >= nav['a_num'][sid_of[i]]:
                    break                                    # the list ends here
                cands.append((F32(s['score'][base + i] + top_lp[base + i, j]), i * k + j, i, a))
        cands.sort(key=lambda c: (-c[0], c[1]))
        sel = cands[:W]
        recs = []
        for q, (sc, _, i, a) in enumerate(sel):
            psid = sid_of[i]
            nxt = int(nav['next_row'][psid, a])
            stay = a == 0 or nxt == psid // V
            nsid = psid if stay else nxt * V + int(nav['cand_view'][psid, a])
            recs.append((q, sc, i, a, psid, nsid, a == 0 or t == E - 1))
        cont = [r for r in recs if not r[6]]
        fins = [r for r in recs if r[6]]
        for p, (q, sc, i, a, psid, nsid, _) in enumerate(cont + fins):
            h = base + p
            s['hist_parent'][t, h], s['hist_action'][t, h], s['hist_rank'][t, h] = base + i, a, q
            s['hist_sid'][t, h], s['hist_psid'][t, h], s['hist_score'][t, h] = nsid, psid, sc
        for d, (q, sc, *_rest) in enumerate(fins):
            s['done_rec'][b, n_done + d] = t * R + base + len(cont) + d
            s['done_score'][b, n_done + d] = sc
        if s['hist_attn'] is not None:
            s['hist_attn'][t, base:base + live] = alpha[base:base + live]
        done_after = n_done + len(fins)
        live_next = 0 if done_after >= W else len(cont)
        if live_next > 0:
            for p, (q, sc, i, a, psid, nsid, _) in enumerate(cont):
                s['row'][base + p], s['view'][base + p] = nsid // V, nsid % V
                s['row'][R + base + p], s['view'][R + base + p] = psid // V, psid % V
                s['act'][base + p], s['parent'][base + p], s['score'][base + p] = a, base + i, sc
        s['act'][base + live_next:base + W] = 0
        s['parent'][base + live_next:base + W] = -1
        s['score'][base + live_next:base + W] = 0
        s['inst'][b] = live_next, done_after, t + 1
        s['live_total'][t] += live_next


def history_of(s):
    """The model's buffers as DeviceFollowerBeam.run returns them."""
    t_end = int(s['inst'][:, 2].max())
    out = dict(inst=s['inst'], done_rec=s['done_rec'], done_score=s['done_score'])
    for name in ('parent', 'action', 'rank', 'sid', 'psid', 'score'):
        out[name] = s['hist_' + name][:t_end]
    out['attn'] = s['hist_attn'][:t_end]
    return out


# ------------------------------------------------------------------------- a synthetic world and stand-in decoder
def synthetic_nav(seed, n_rows=9, A=6):
    """Navigation tables with short candidate lists, moves that stay in place and states with one candidate only."""
    rng = np.random.default_rng(seed)
    n = n_rows * V
    a_num = rng.integers(1, A + 1, n).astype(np.int32)
    own = np.repeat(np.arange(n_rows), V)
    next_row = rng.integers(0, n_rows, (n, A)).astype(np.int32)
    next_row[rng.random((n, A)) < 0.15] = -1
    next_row = np.where(next_row < 0, own[:, None], next_row).astype(np.int32)      # a candidate on the own viewpoint
    next_row[:, 0] = own
    cand_view = rng.integers(0, V, (n, A)).astype(np.int32)
    cand_view[:, 0] = 0
    return dict(a_num=a_num, next_row=next_row, cand_view=cand_view, feat_row=np.arange(n_rows, dtype=np.int32),
                sincos=np.zeros((n, A, 4), F32)), A


def history_logp(hist, A, depth_bias=4):
    rng = np.random.default_rng(zlib.crc32(np.asarray(hist, np.int64).tobytes()))
    lp = (-0.5 * rng.integers(0, 5, A)).astype(F32)                  # coarse steps: many exact ties, exact sums
    lp[0] = F32(-0.5 * max(depth_bias - len(hist), 0))               # stopping gets likelier as the route grows
    return lp


def history_alpha(hist, T):
    rng = np.random.default_rng(zlib.crc32(np.asarray(hist, np.int64).tobytes()) ^ 0x5bd1)
    return rng.random(T).astype(F32)


def topk_valid(lp, n_valid, k):
    """sf_logprob_topk with n_valid (include/sf_hip.h): the stable descending sort of the masked row -- descending,
    ties lower column first, and past the valid columns the masked ones in column order as (column, -inf)."""
    masked = np.where(np.arange(len(lp)) < n_valid, lp, F32(-np.inf)).astype(F32)
    o = np.lexsort((np.arange(len(lp)), -masked))[:k]
    return o.astype(np.int32), masked[o]


TT = 5                            # attention row width of the stand-in


class FakeFlatDecoder:
    """search.FlatDecoder's step_arrays over history_logp: pool row -> the states its hypothesis went through."""

    def __init__(self, nav, A, B):
        self.nav, self.A = nav, A
        self.hist = {b: (-1 - b,) for b in range(B)}
        self.att = {}
        self.n = B

    def step_arrays(self, inp, k):
        N = len(inp['vp'])
        k = min(k, int(inp['a_num'].max()))                # (what FlatDecoder does: A = the widest list of the step)
        base = self.n
        ta, tl = np.zeros((N, k), np.int64), np.zeros((N, k), F32)
        for i in range(N):
            sid = int(inp['vp'][i]) * V + int(inp['view'][i])
            h = self.hist[int(inp['hrow'][i])] + (sid,)
            self.hist[base + i] = h
            self.att[base + i] = history_alpha(h, TT)
            ta[i], tl[i] = topk_valid(history_logp(h, self.A), int(self.nav['a_num'][sid]), k)
        self.n += N
        return base, ta, tl

    def attention_rows(self, rows):
        return [self.att[int(r)].copy() for r in rows]


def fake_space(nav, B, seed):
    from speaker_follower_amd import frontier
    rng = np.random.default_rng(seed)
    n_rows = len(nav['feat_row'])
    sp = frontier.StateSpace.__new__(frontier.StateSpace)
    sp.h, sp.key_fields = nav, 4
    sp.items = [dict(instr_id='i%d' % b, instr_encoding=[b, b + 1]) for b in range(B)]
    sp.base_row = np.zeros(B, np.int64)
    sp.root_sid = rng.integers(0, n_rows * V, B).astype(np.int64)
    sp.n_keys = n_rows * V + 2
    sp.root_key = np.full(B, sp.n_keys - 1, np.int64)
    sp.env = sp.nav = None
    sp._obs = {}
    return sp


class FakeAgent:
    def __init__(self, episode_len):
        self.episode_len = episode_len


def host_loop(monkeypatch, nav, A, B, beam, E, seed, tie_log=None):
    """frontier.beam_search over the stand-in decoder.  Returns (result triple, hypothesis table, decoder)."""
    from speaker_follower_amd import frontier
    sp = fake_space(nav, B, seed)
    fd = FakeFlatDecoder(nav, A, B)
    t = frontier.Hypotheses()
    roots = t.append(np.zeros(B, F32), np.ones(B, bool), parent=-1, inst=np.arange(B), sid=sp.root_sid,
                     key=sp.root_key, action=-1, count=0, pool=np.arange(B))
    env = type('E', (), {'beam_size': beam})()
    monkeypatch.setattr(frontier, '_setup', lambda agent, load: (env, sp, fd, t, roots))
    agent = FakeAgent(E)
    if tie_log is not None:
        agent.tie_log = tie_log
    return frontier.beam_search(agent, beam), t, fd, sp


def device_model(nav, A, B, beam, E, sp):
    """The device step loop with the decoder replaced by history_logp: DeviceFollowerBeam.run's result."""
    R, k = B * beam, min(beam, A)
    s = new_state(B, beam, E, TT, sp.root_sid)
    hist = {b * beam: (-1 - b,) for b in range(B)}            # slot -> states its PARENT hypothesis went through
    for _ in range(E + 2):                                    # (steps past the end change nothing)
        top_a, top_lp = np.full((R, k), -1, np.int32), np.full((R, k), -np.inf, F32)
        alpha = np.full((R, TT), np.nan, F32)
        cur = {}
        for b in range(B):
            for i in range(int(s['inst'][b, 0])):
                r = b * beam + i
                sid = int(s['row'][r]) * V + int(s['view'][r])
                cur[r] = hist[int(s['parent'][r])] + (sid,)
                alpha[r] = history_alpha(cur[r], TT)
                top_a[r], top_lp[r] = topk_valid(history_logp(cur[r], A), int(nav['a_num'][sid]), k)
        model_step(s, nav, top_a, top_lp, alpha)
        hist = cur                                            # the next step's parents are this step's slots
    return history_of(s)


def cand_fields(c):
    return {k: c[k] for k in ('instr_id', 'instr_encoding', 'actions', 'score', 'scores')}


def assert_same_results(got, want):
    assert len(got[0]) == len(want[0])
    for gl, wl in zip(got[0], want[0]):
        assert len(gl) == len(wl)
        for g, w in zip(gl, wl):
            assert cand_fields(g) == cand_fields(w)
            assert len(g['attentions']) == len(w['attentions'])
            for x, y in zip(g['attentions'], w['attentions']):
                assert x.dtype == y.dtype and np.array_equal(x, y)
    assert [h.nodes for h in got[1]] == [h.nodes for h in want[1]]
    assert got[2] is None and want[2] is None


# ---------------------------------------------------------------------------------------------------- the tests
def test_shared_tail_matches_the_literal_host_tail_with_ties():
    """frontier.beam_outputs against the last five lines of frontier.beam_search as they stood before it was shared."""
    from speaker_follower_amd import frontier
    rng = np.random.default_rng(11)
    B, beam, depth = 4, 3, 6
    nav, A = synthetic_nav(2)
    sp = fake_space(nav, B, 5)
    t = frontier.Hypotheses()
    t.append(np.zeros(B, F32), np.ones(B, bool), parent=-1, inst=np.arange(B), sid=sp.root_sid, key=sp.root_key,
             action=-1, count=0, pool=np.arange(B))
    for n in range(B, 160):                                   # a random forest, at most `depth` deep
        p = int(rng.integers(0, n))
        while t.count[p] >= depth:
            p = int(t.parent[p])
        t.append(np.array([F32(t.score[p] + F32(-0.5 * rng.integers(0, 3)))]), np.array([False]), parent=p,
                 inst=t.inst[p], sid=int(rng.integers(0, len(nav['a_num']))), key=0, action=int(rng.integers(0, A)),
                 count=t.count[p] + 1, pool=n)
    att = rng.random((160, TT)).astype(F32)
    fd = type('FD', (), {'attention_rows': staticmethod(lambda rows: [att[r].copy() for r in rows])})()
    done = [[int(n) for n in rng.permutation(np.flatnonzero((t.inst[:160] == b) & (t.parent[:160] >= 0)))[:8]]
            for b in range(B)]
    assert any(len(set(t.score[d].tolist())) < len(d) for d in done), 'no exact ties in the synthetic completions'
    # the literal restatement
    best = []
    for lst in done:
        sc = t.score[lst]
        best.append([lst[i] for i in np.lexsort((np.arange(len(lst)), -sc))[:beam]])
    want = (frontier._trajectories(fd, t, sp, best, depth), [frontier.HypList(t, sp, lst) for lst in done], None)
    log = []
    got = frontier.beam_outputs(fd, t, sp, done, beam, depth, log)
    assert_same_results(got, want)
    assert_same_results(frontier.beam_outputs(fd, t, sp, done, beam, depth), want)
    assert [x[1] for x in log] == list(range(B)) and all(x[0] == 'rank' and (x[2] >= 0).all() for x in log)
    hyp = got[1][0][0]
    assert hyp.score == float(t.score[done[0][0]]) and hyp.last_action == int(t.action[done[0][0]])
    assert hyp.prev_inference_state.node == int(t.parent[done[0][0]])


@pytest.mark.parametrize('B,beam,E,seed', [(3, 4, 6, 1), (5, 3, 8, 2), (2, 1, 5, 3), (4, 12, 5, 4), (3, 7, 3, 5)])
def test_device_history_layout_gives_the_host_loop_table_node_for_node(monkeypatch, B, beam, E, seed):
    from speaker_follower_amd import frontier
    nav, A = synthetic_nav(seed)
    want, t_host, fd, sp = host_loop(monkeypatch, nav, A, B, beam, E, seed)
    hist = device_model(nav, A, B, beam, E, sp)
    t_dev, done = frontier.hypotheses_from_history(sp, hist, beam)
    assert t_dev.n == t_host.n > B
    for f in ('parent', 'inst', 'sid', 'key', 'action', 'count', 'score', 'start_pose'):
        assert np.array_equal(getattr(t_dev, f)[:t_dev.n], getattr(t_host, f)[:t_host.n]), f
    assert t_dev.score.dtype == np.float32
    att = hist['attn'].reshape(-1, TT)
    for n in range(B, t_dev.n):                               # the same attention row behind every node's pool row
        assert np.array_equal(att[t_dev.pool[n]], fd.att[int(t_host.pool[n])]), n
    assert done == [h.nodes for h in want[1]]
    got = frontier.beam_outputs(frontier.HistoryAttention(att), t_dev, sp, done, beam, E)
    assert_same_results(got, want)
    # what the synthetic world is there for
    sc = t_host.score[B:t_host.n]
    assert len(np.unique(sc)) < len(sc), 'no exact score ties'
    assert (t_host.sid[B:t_host.n] == t_host.sid[t_host.parent[B:t_host.n]]).any(), 'no successor stays in place'
    assert (nav['a_num'][t_host.sid[:t_host.n]] < min(beam, A)).any() or beam == 1, 'no short candidate list'
    assert (hist['inst'][:, 1] >= 1).all()


def test_instances_end_at_different_steps_and_stop_when_their_completions_are_full(monkeypatch):
    nav, A = synthetic_nav(7)
    B, beam, E = 6, 2, 9
    want, t_host, fd, sp = host_loop(monkeypatch, nav, A, B, beam, E, 7)
    hist = device_model(nav, A, B, beam, E, sp)
    ends = hist['inst'][:, 2]
    assert len(set(ends.tolist())) > 1, ends
    full = hist['inst'][:, 1] >= beam
    assert full.any() and (hist['inst'][full, 0] == 0).all()


def test_margin_log_records_gaps_and_changes_nothing(monkeypatch):
    nav, A = synthetic_nav(1)
    plain, t0, _, _ = host_loop(monkeypatch, nav, A, 3, 4, 6, 1)
    log = []
    logged, t1, _, _ = host_loop(monkeypatch, nav, A, 3, 4, 6, 1, tie_log=log)
    assert_same_results(logged, plain)
    assert t0.n == t1.n and np.array_equal(t0.score[:t0.n], t1.score[:t1.n])
    sel = [x for x in log if x[0] == 'select']
    rank = [x for x in log if x[0] == 'rank']
    assert sel and len(rank) == 3
    for _, step, inst, gap in sel:
        assert 0 <= step < 6 and len(inst) == len(gap) and gap.dtype == np.float32 and (gap >= 0).all()
    assert any((gap == 0).any() for _, _, _, gap in sel), 'the synthetic world has exact ties at the cut'
    for _, b, gap in rank:
        assert (gap >= 0).all() and gap.dtype == np.float32


# ---- the C entry
def _fol_struct(lib_mod, B=4, beam=8, k=6, E=10, T=5, A=6, ld=None, nulls=(), nav_nulls=()):
    R = B * beam
    navp = dict(a_num=64, next_row=64, cand_view=64, cand_sincos=64, feat_row=64)
    for n in nav_nulls:
        navp[n] = None
    nav = lib_mod.NavTableS(navp['a_num'], navp['next_row'], navp['cand_view'], navp['cand_sincos'], navp['feat_row'],
                            A, V)
    names = ('score', 'row', 'view', 'act', 'parent', 'inst', 'live_total', 'hist_parent', 'hist_action', 'hist_rank',
             'hist_sid', 'hist_psid', 'hist_score', 'hist_attn')
    f = {n: 64 for n in names + ('done_rec', 'done_score')}
    for n in nulls:
        f[n] = None
    return lib_mod.FolBeam(B, beam, k, E, T, 0, nav, *(f[n] for n in names), R * (6 + T) if ld is None else ld,
                           f['done_rec'], f['done_score'])


def test_follower_beam_select_entry_is_exported_and_bound():
    from speaker_follower_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'sf_follower_beam_select')
    assert 'sf_follower_beam_select' in _lib.EXPORTS
    assert _lib.lib.sf_follower_beam_select.argtypes is not None
    assert _lib.ABI_VERSION == 10 and _lib.lib.sf_abi_version() == 10


def test_follower_beam_select_rejects_bad_arguments_without_gpu():
    """Pointers that look valid (never dereferenced: the checks come first), then one bad argument at a time."""
    from speaker_follower_amd import _lib
    sel = _lib.lib.sf_follower_beam_select
    dev = C.c_void_p(64)
    assert sel(None, dev, dev, dev, None) == _lib.SF_ERR_ARG
    s = _fol_struct(_lib)
    assert sel(C.byref(s), None, dev, dev, None) == _lib.SF_ERR_ARG                      # top_a
    assert sel(C.byref(s), dev, None, dev, None) == _lib.SF_ERR_ARG                      # top_lp
    assert sel(C.byref(s), dev, dev, None, None) == _lib.SF_ERR_ARG                      # hist_attn without alpha
    for n in ('score', 'row', 'view', 'act', 'parent', 'inst', 'live_total', 'hist_parent', 'hist_action', 'hist_rank',
              'hist_sid', 'hist_psid', 'hist_score', 'done_rec', 'done_score'):
        s = _fol_struct(_lib, nulls=(n,))
        assert sel(C.byref(s), dev, dev, dev, None) == _lib.SF_ERR_ARG, n
    for n in ('a_num', 'next_row', 'cand_view'):
        s = _fol_struct(_lib, nav_nulls=(n,))
        assert sel(C.byref(s), dev, dev, dev, None) == _lib.SF_ERR_ARG, n
    for kw in (dict(k=9, beam=8, A=12), dict(k=7, A=6), dict(k=0), dict(B=0), dict(beam=0, k=0), dict(E=0), dict(T=0),
               dict(A=0), dict(ld=4 * 8 * 5 - 1), dict(ld=4 * 8 - 1)):
        s = _fol_struct(_lib, **kw)
        assert sel(C.byref(s), dev, dev, dev, None) == _lib.SF_ERR_ARG, kw
    s = _fol_struct(_lib, beam=65, k=65, A=70)                                           # wider than one wavefront
    assert sel(C.byref(s), dev, dev, dev, None) == _lib.SF_ERR_UNSUPPORTED
    s = _fol_struct(_lib, beam=65, k=66, A=70)
    assert sel(C.byref(s), dev, dev, dev, None) == _lib.SF_ERR_ARG


def test_switch_is_off_by_default_and_a_wide_beam_is_not_supported():
    from speaker_follower_amd import agents, search
    assert agents.Seq2SeqAgent.beam_on_device is False and agents.Seq2SeqAgent.beam_fallbacks == 0
    assert search.DeviceFollowerBeam.supports(64) and not search.DeviceFollowerBeam.supports(65)
    assert not search.DeviceFollowerBeam.supports(0)
    assert not search.DeviceFollowerBeam.supports(3, decoder=object())
