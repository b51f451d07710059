"""CPU: the host side of the state-factored search's device loop (search.DeviceStateFactored /
sf_state_factored_select).

* the case table of the kernel test (tests/test_gpu_state_factored_device.py): a synthetic two-scan world
  (test_follower_beam_device_host.synthetic_nav twice), log-probabilities quantised to multiples of 1/8 -- float32 sums
  are exact and ties frequent -- with 1e30 in every column that is no candidate, so a stray read shows up as a wrong pick;
* a step-by-step model of the kernel over the device's table layout (`model_iteration`, which the GPU test holds the
  kernel to word for word), held here to sim/frontier_core.cpp's StateFactored node for node; the model records what
  happened on the way (ties between "open" and "held", groups, replacements, ...) and the cases are asserted to reach
  what they are there for;
* frontier.hypotheses_from_search_tables -- per-instance node ids renumbered to the host loop's, completed order, visits --
  against core.hypotheses() / core.results();
* the C entry rejects bad arguments before touching the device;
* the dispatch rules of Seq2SeqAgent.search_on_device, with a stand-in device search."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_follower_beam_device_host import synthetic_nav          # noqa: E402

F32 = np.float32
V = 36
NEG_INF_BITS = int(np.array(-np.inf, F32).view(np.int32))
NODE_FIELDS = ('parent', 'sid', 'key', 'action', 'count', 'pool', 'start', 'born', 'score')

# (B, successor_size, completion_size, episode_len, key_fields)
CASES = [(1, 1, 1, 2, 4), (3, 1, 3, 6, 4), (5, 2, 4, 6, 3), (7, 3, 5, 4, 2), (2, 1, 2, 3, 1), (64, 1, 40, 8, 4)]
ROWS = 9                          # viewpoints per scan of the synthetic world


def case_id(c):
    return 'B%d_s%d_c%d_e%d_k%d' % c


# ------------------------------------------------------------------------------------------- the synthetic world
def two_scan_world(case):
    """Two synthetic scans back to back (instances alternate between them: base_row 0 and ROWS), roots drawn per case."""
    B, S, comp, E, kf = case
    seed = 1000 * B + 100 * S + 10 * comp + kf
    (n0, A), (n1, _) = synthetic_nav(seed), synthetic_nav(seed + 1)
    nav = {k: np.concatenate((n0[k], n1[k])) for k in ('a_num', 'cand_view', 'sincos')}
    nav['next_row'] = np.concatenate((n0['next_row'], n1['next_row'] + ROWS)).astype(np.int32)
    nav['feat_row'] = np.arange(2 * ROWS, dtype=np.int32)
    rng = np.random.default_rng(seed + 2)
    scan = np.arange(B) % 2
    base_row = (scan * ROWS).astype(np.int64)
    root_sid = (base_row + rng.integers(0, ROWS, B)) * V + rng.integers(0, V, B)
    per = {4: V, 3: 12, 2: 1, 1: 0}[kf]
    n_keys = ROWS * per + 2
    local = root_sid // V - base_row
    root_key = (np.full(B, n_keys - 1, np.int64) if kf >= 3 else local if kf == 2 else np.zeros(B, np.int64))
    return dict(nav=nav, A=A, base_row=base_row, root_sid=root_sid.astype(np.int64), root_key=root_key.astype(np.int64),
                n_keys=n_keys, seed=seed)


def host_core(case, world):
    from speaker_follower_amd.sim import load_frontier
    B, S, comp, E, kf = case
    nav = world['nav']
    return load_frontier().StateFactored(comp, S, E, kf, V, nav['next_row'], nav['cand_view'], nav['a_num'],
                                         world['base_row'], world['root_sid'], world['root_key'])


def synthetic_logp(world, iteration, block, n, cap):
    """[cap, A] float32 for one iteration: multiples of 1/8 in the candidate columns of the n frontier rows (a function of
    the world, the iteration and the row), 1e30 everywhere else."""
    A, nav = world['A'], world['nav']
    rng = np.random.default_rng((world['seed'], iteration))
    # (a few values above zero -- no log-probability, but the bookkeeping is defined for any float: a later successor
    # can then beat a state that was already completed)
    lp = ((2 - rng.integers(0, 14, (cap, A))) / 8.0).astype(F32)
    sid = block[0, :cap].astype(np.int64) * V + block[2, :cap]
    lp[np.arange(A)[None, :] >= nav['a_num'][sid][:, None]] = F32(1e30)
    lp[n:] = F32(1e30)
    return lp


# ------------------------------------------------------------------------------------- the kernel's model and tables
def new_tables(case, world, node_cap, slot_cap, visit_cap, base, pool_rows=1 << 20):
    """The tables of sf_state_search as DeviceStateFactored.initial_tables presets them, one numpy array per pointer."""
    B, S, comp, E, kf = case
    K, cap = world['n_keys'], B * S
    T = dict(B=B, S=S, comp=comp, E=E, kf=kf, K=K, node_cap=node_cap, slot_cap=slot_cap, visit_cap=visit_cap, cap=cap,
             pool_rows=pool_rows, status=np.zeros(8, np.int32), inst=np.zeros((B, 8), np.int32),
             frontier=np.zeros((B, S), np.int32), base_row=world['base_row'].astype(np.int32),
             comp_order=np.zeros((B, comp + S), np.int32), visits=np.zeros((B, visit_cap), np.int32),
             comp_node=np.full((B, K), -1, np.int32), dev_in=np.zeros((8, cap), np.int32))
    for f in NODE_FIELDS:
        T['node_' + f] = np.zeros((B, node_cap), F32 if f == 'score' else np.int32)
    for d in ('open', 'held'):
        T[d + '_slot'] = np.full((B, K), -1, np.int32)
        T[d + '_key'], T[d + '_node'] = np.zeros((B, slot_cap), np.int32), np.zeros((B, slot_cap), np.int32)
        T[d + '_pick'] = np.zeros((B, slot_cap), F32)
    b = np.arange(B)
    root = b * node_cap
    T['status'][:2] = B, base
    T['inst'][:, [0, 1, 4, 5]] = 1
    T['inst'][:, 6] = b
    T['frontier'][:, 0] = root
    T['visits'][:, 0] = root
    T['node_parent'][:, 0], T['node_action'][:, 0] = -1, -1
    T['node_sid'][:, 0], T['node_key'][:, 0] = world['root_sid'], world['root_key']
    T['node_pool'][:, 0], T['node_start'][:, 0] = b, 1
    T['open_slot'][b, world['root_key']] = 0
    T['open_key'][:, 0], T['open_node'][:, 0], T['open_pick'][:, 0] = world['root_key'], root, -np.inf
    _model_pack_columns(T, list(root), base)
    return T


def _model_pack_columns(T, frontier, base):
    cap, nc = T['cap'], T['node_cap']
    flat = {f: T['node_' + f].reshape(-1) for f in NODE_FIELDS}
    head = frontier[0] if frontier else 0
    for i in range(cap):
        f = frontier[i] if i < len(frontier) else head
        s, p = int(flat['sid'][f]), int(flat['parent'][f])
        ps = int(flat['sid'][p]) if p >= 0 else s
        T['dev_in'][:, i] = (s // V, ps // V, s % V, ps % V, int(flat['action'][f]) if p >= 0 else 0, flat['pool'][f],
                             f // nc, base + i if i < len(frontier) else -1)


def model_iteration(T, nav, A, logp, events=None):
    """One call of sf_state_factored_select (include/sf_hip.h) on the tables `T`, in place.  logp [cap, >= A] float32.
    events: a dict that counts what happened, or None."""
    ev = events if events is not None else {}

    def note(name):
        ev[name] = ev.get(name, 0) + 1

    B, S, K, nc = T['B'], T['S'], T['K'], T['node_cap']
    st = T['status']
    if st[0] <= 0 or st[3] != 0:
        return
    base, born = int(st[1]), int(st[2]) + 1
    flat = {f: T['node_' + f].reshape(-1) for f in NODE_FIELDS}
    for b in range(B):
        n_nodes, n_open, n_held, n_comp, n_vis, nf, first, _ = (int(x) for x in T['inst'][b])
        if n_comp >= T['comp']:
            continue
        n_slots = dict(open=n_open, held=n_held)
        succ = []
        for r in range(nf):
            f = int(T['frontier'][b, r])
            sid = int(flat['sid'][f])
            for a in range(min(int(nav['a_num'][sid]), A)):
                succ.append((F32(flat['score'][f] + logp[first + r, a]), r * A + a, r, a, f, sid))
        succ.sort(key=lambda x: (-x[0], x[1]))
        seen, new, fresh, bad_key = set(), [], dict(open=0, held=0), False
        for score, _, r, a, f, sid in succ:
            nxt = int(nav['next_row'][sid, a])
            stay = a == 0 or nxt == sid // V
            nsid = sid if stay else nxt * V + int(nav['cand_view'][sid, a])
            if stay:
                key = int(flat['key'][f])
            else:
                local = nsid // V - int(T['base_row'][b])
                key = {4: local * V + nsid % V, 3: local * 12 + nsid % 12, 2: local, 1: 0}[T['kf']]
            count = int(flat['count'][f]) + 1
            final = a == 0 or count == T['E']
            if final and a != 0:
                note('final by the episode length')
            bad_key |= not 0 <= key < K
            if (key, final) in seen:
                note('second successor of a (key, final) group')
                continue
            seen.add((key, final))
            d = 'held' if final else 'open'
            slot = -1 if bad_key else int(T[d + '_slot'][b, key])
            if slot >= 0 and not flat['score'][T[d + '_node'][b, slot]] < score:
                continue
            if slot >= 0:
                note('replacement in ' + d)
            else:
                fresh[d] += 1
            new.append((d, key, slot, f, nsid, a, count, base + first + r, score, bool(flat['start'][f]) and stay))
        if bad_key:
            T['inst'][b, 7] |= 16
            continue
        ovf = (1 if n_nodes + len(new) > nc else 0) | \
              (2 if max(n_open + fresh['open'], n_held + fresh['held']) > T['slot_cap'] else 0)
        if ovf:
            T['inst'][b, 7] |= ovf
            continue
        for d, key, slot, f, nsid, a, count, pool, score, start in new:
            nid = b * nc + n_nodes
            n_nodes += 1
            for name, val in zip(NODE_FIELDS, (f, nsid, key, a, count, pool, int(start), born, score)):
                flat[name][nid] = val
            if slot < 0:
                slot = n_slots[d]
                n_slots[d] += 1
                T[d + '_slot'][b, key], T[d + '_key'][b, slot] = slot, key
            T[d + '_node'][b, slot], T[d + '_pick'][b, slot] = nid, score
        if max(n_slots.values()) > 64:
            note('a dictionary with more than 64 slots')
        picks = []
        for _ in range(S):
            best = {}
            for d in ('open', 'held'):
                p = T[d + '_pick'][b, :n_slots[d]]
                i = int(np.argmax(p)) if len(p) else -1
                best[d] = (i, p[i]) if i >= 0 and p[i] > -np.inf else (-1, F32(-np.inf))
            if best['open'][0] < 0 and best['held'][0] < 0:
                break
            if best['open'][0] >= 0 and best['held'][0] >= 0 and best['open'][1] == best['held'][1]:
                note('exact tie between open and held')
            d = 'held' if best['held'][1] > best['open'][1] else 'open'
            slot = best[d][0]
            T[d + '_pick'][b, slot] = -np.inf
            picks.append((int(T[d + '_key'][b, slot]), int(T[d + '_node'][b, slot]), d == 'held'))
        for key, node, held in picks:
            if not held:
                continue
            old = int(T['comp_node'][b, key])
            if old < 0:
                T['comp_node'][b, key] = node
                T['comp_order'][b, n_comp] = key
                n_comp += 1
            elif flat['score'][old] < flat['score'][node]:
                T['comp_node'][b, key] = node
                note('a completed state improved')
        cnt, ovf = 0, 0
        for key, node, held in picks:
            if held or n_comp >= T['comp']:
                continue
            if n_vis >= T['visit_cap']:
                ovf = 4
                break
            T['frontier'][b, cnt] = node
            T['visits'][b, n_vis] = node
            cnt, n_vis = cnt + 1, n_vis + 1
        if not picks and n_comp < T['comp']:
            note('an instance ran out of states')
        T['inst'][b, :6] = n_nodes, n_slots['open'], n_slots['held'], n_comp, n_vis, cnt
        T['inst'][b, 7] |= ovf
    # ---- the pack launch
    flags = int(np.bitwise_or.reduce(T['inst'][:, 7]))
    cnt = T['inst'][:, 5].copy()
    base += int(st[0])
    if not flags and cnt.sum() > 0 and base + cnt.sum() > T['pool_rows']:
        flags = 8
    T['inst'][:, 6] = np.cumsum(cnt) - cnt
    if flags:
        T['inst'][:, 5] = cnt = np.zeros_like(cnt)
    _model_pack_columns(T, [int(T['frontier'][b, j]) for b in range(B) for j in range(cnt[b])], base)
    st[0], st[1], st[2], st[3] = cnt.sum(), base, st[2] + 1, flags


def tables_for_assembly(T):
    """The model's (or the device's) tables as DeviceStateFactored.run hands them to the assembly."""
    comp = np.take_along_axis(T['comp_node'], np.clip(T['comp_order'], 0, T['K'] - 1).astype(np.int64), axis=1)
    return dict(node_cap=T['node_cap'], inst=T['inst'], comp=comp, visits=T['visits'],
                **{f: T['node_' + f] for f in NODE_FIELDS})


def run_host_and_model(case, node_cap=4096, slot_cap=1024, extra_iterations=0, on_iteration=None):
    """The same synthetic log-probabilities through StateFactored.advance and through the model.  Returns (core, tables,
    events, iterations)."""
    world = two_scan_world(case)
    B, S = case[0], case[1]
    cap = B * S
    core = host_core(case, world)
    T = new_tables(case, world, node_cap, slot_cap, node_cap, base=B)
    events, block, base, it = {}, np.zeros((8, cap), np.int32), B, 0
    while True:
        n = core.fill_inputs(block, base)
        assert np.array_equal(T['dev_in'], block), it
        assert (int(T['status'][0]), int(T['status'][1])) == (n, base)
        lp = synthetic_logp(world, it, block, n, cap)
        nxt = core.advance(lp, base)
        model_iteration(T, world['nav'], world['A'], lp, events)
        if on_iteration is not None:
            on_iteration(it, lp, T)
        base += n
        it += 1
        assert int(T['status'][0]) == nxt and int(T['status'][1]) == base and int(T['status'][3]) == 0
        if nxt == 0 or core.done():
            break
    assert int(T['status'][0]) == 0 and int(T['status'][2]) == it
    return core, T, events, it


def assert_same_as_core(core, T, case):
    from speaker_follower_amd import frontier
    B, comp = case[0], case[2]
    t, completed, visits = frontier.hypotheses_from_search_tables(tables_for_assembly(T), B, comp)
    want = frontier.Hypotheses.from_arrays(*core.hypotheses())
    assert t.n == want.n >= B
    for f in ('parent', 'inst', 'sid', 'key', 'action', 'count', 'pool', 'start_pose'):
        assert np.array_equal(getattr(t, f), getattr(want, f)), f
    assert t.score.dtype == np.float32 and np.array_equal(t.score.view(np.int32), want.score.view(np.int32))
    want_completed, want_visits = core.results()
    assert completed == [list(x) for x in want_completed]
    assert visits == [list(x) for x in want_visits]
    return t


# ---------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope='module')
def runs():
    return {c: run_host_and_model(c) for c in CASES}


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_model_and_assembly_give_the_host_loop_table_node_for_node(runs, case):
    core, T, events, it = runs[case]
    t = assert_same_as_core(core, T, case)
    assert it >= 1 and t.n > case[0]
    sc = t.score[case[0]:]
    assert np.array_equal(sc, np.round(sc * 8) / 8), 'the sums are not exact'


def test_cases_reach_what_they_are_there_for(runs):
    total = {}
    for c in CASES:
        for k, v in runs[c][2].items():
            total[k] = total.get(k, 0) + v
    for what in ('exact tie between open and held', 'second successor of a (key, final) group', 'replacement in held',
                 'replacement in open', 'a completed state improved', 'an instance ran out of states',
                 'a dictionary with more than 64 slots', 'final by the episode length'):
        assert total.get(what, 0) > 0, (what, total)
    # instances of one search finish at different iterations: their visit counts differ while all have their completions
    core, T, _, _ = runs[(3, 1, 3, 6, 4)]
    done = T['inst'][:, 3] >= 3
    assert len(set(T['inst'][done, 4].tolist())) > 1 or not done.all(), T['inst']
    big = runs[(64, 1, 40, 8, 4)][1]
    assert len(set(big['inst'][:, 4].tolist())) > 4
    assert big['inst'][:, 1].max() > 64 and runs[(64, 1, 40, 8, 4)][3] > 40


def test_an_iteration_with_an_empty_frontier_changes_nothing():
    case = (3, 1, 3, 6, 4)
    world = two_scan_world(case)
    _, T, _, _ = run_host_and_model(case)
    before = {k: v.copy() for k, v in T.items() if isinstance(v, np.ndarray)}
    for _ in range(3):
        model_iteration(T, world['nav'], world['A'], np.full((3, world['A']), 1e30, F32))
    for k, v in before.items():
        assert np.array_equal(T[k], v), k


@pytest.mark.parametrize('which', ['slot_cap', 'node_cap'])
def test_model_overflow_sets_the_flag_and_empties_the_frontier(runs, which):
    case = (3, 1, 3, 6, 4)
    _, T, _, _ = runs[case]
    need = dict(slot_cap=int(T['inst'][:, 1:3].max()), node_cap=int(T['inst'][:, 0].max()))
    world = two_scan_world(case)
    caps = dict(node_cap=4096, slot_cap=1024)
    caps[which] = need[which] - 1
    M = new_tables(case, world, caps['node_cap'], caps['slot_cap'], 4096, base=3)
    for it in range(200):
        if M['status'][0] == 0:
            break
        lp = synthetic_logp(world, it, M['dev_in'], int(M['status'][0]), 3)
        model_iteration(M, world['nav'], world['A'], lp)
    assert M['status'][0] == 0 and M['status'][3] == (2 if which == 'slot_cap' else 1)
    assert (M['dev_in'][7] == -1).all() and (M['inst'][:, 5] == 0).all()


# ---- the C entry
def _search_struct(lib_mod, nulls=(), nav_nulls=(), A=6, **sizes):
    z = dict(B=4, successor_size=2, completion_size=3, episode_len=6, key_fields=4, n_keys=100, node_cap=64, slot_cap=32,
             visit_cap=64, cap=8, pool_rows=1024, reserved=0)
    z.update(sizes)
    navp = dict(a_num=64, next_row=64, cand_view=64, cand_sincos=64, feat_row=64)
    for n in nav_nulls:
        navp[n] = None
    nav = lib_mod.NavTableS(navp['a_num'], navp['next_row'], navp['cand_view'], navp['cand_sincos'], navp['feat_row'], A, V)
    p = {n: 64 for n in lib_mod.StateSearch.POINTERS}
    for n in nulls:
        p[n] = None
    return lib_mod.StateSearch(*(z[n] for n in lib_mod.StateSearch.SIZES), nav,
                               *(p[n] for n in lib_mod.StateSearch.POINTERS))


def test_state_factored_select_entry_is_exported_and_bound():
    from speaker_follower_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'sf_state_factored_select')
    assert 'sf_state_factored_select' in _lib.EXPORTS
    assert _lib.lib.sf_state_factored_select.argtypes is not None
    assert _lib.ABI_VERSION == 10 and _lib.lib.sf_abi_version() == 10           # (an added function; 10 is the removal of the retired schedules' fields)
    assert C.sizeof(_lib.StateSearch) == 12 * 4 + C.sizeof(_lib.NavTableS) + 24 * 8


def test_state_factored_select_rejects_bad_arguments_without_gpu():
    """Pointers that look valid (never dereferenced: the checks come first), then one bad argument at a time."""
    from speaker_follower_amd import _lib
    sel = _lib.lib.sf_state_factored_select
    dev = C.c_void_p(64)
    s = _search_struct(_lib)
    assert sel(None, dev, 6, dev, None) == _lib.SF_ERR_ARG
    assert sel(C.byref(s), None, 6, dev, None) == _lib.SF_ERR_ARG                        # logp
    assert sel(C.byref(s), dev, 6, None, None) == _lib.SF_ERR_ARG                        # dev_in
    assert sel(C.byref(s), dev, 5, dev, None) == _lib.SF_ERR_ARG                         # ld_logp < A
    for n in _lib.StateSearch.POINTERS:
        s = _search_struct(_lib, nulls=(n,))
        assert sel(C.byref(s), dev, 6, dev, None) == _lib.SF_ERR_ARG, n
    for n in ('a_num', 'next_row', 'cand_view'):
        s = _search_struct(_lib, nav_nulls=(n,))
        assert sel(C.byref(s), dev, 6, dev, None) == _lib.SF_ERR_ARG, n
    for kw in (dict(B=0), dict(successor_size=0), dict(completion_size=0), dict(episode_len=0), dict(key_fields=0),
               dict(key_fields=5), dict(n_keys=0), dict(node_cap=0), dict(slot_cap=0), dict(visit_cap=0), dict(pool_rows=0),
               dict(cap=7), dict(A=0), dict(B=128, cap=256, node_cap=1 << 24)):
        s = _search_struct(_lib, **kw)
        assert sel(C.byref(s), dev, 6, dev, None) == _lib.SF_ERR_ARG, kw
    # beyond the lane mapping: successor_size * A > 1024, successor_size > 64, B > 256
    for kw, ld in ((dict(successor_size=64, cap=256, A=17), 17), (dict(successor_size=65, cap=260, A=2), 6),
                   (dict(B=257, cap=514), 6)):
        s = _search_struct(_lib, **kw)
        assert sel(C.byref(s), dev, ld, dev, None) == _lib.SF_ERR_UNSUPPORTED, kw
    # the limits themselves are argument-clean (nothing is launched here: the next check would be the launch itself)
    from speaker_follower_amd import search
    D = search.DeviceStateFactored
    assert D.supports(64, 256, 16) and not D.supports(64, 256, 17) and not D.supports(65, 1, 1)
    assert not D.supports(1, 257, 6) and D.supports(1, 128, 15) and not D.supports(0)
    assert not D.supports(1, 8, 6, decoder=object())


# ---- the switch
class _FakeAgent:
    search_on_device = True
    search_fallbacks = 0
    search_backend = 'native'
    store = object()

    def __init__(self, visual=True):
        self.decoder = type('Dec', (), {'visual_attention_layer': None} if visual else {})()


def _patched(monkeypatch, device_result, shape=(8, 6)):
    from speaker_follower_amd import search, frontier
    calls = []
    monkeypatch.setattr(search, '_search_shape', lambda agent: shape)
    monkeypatch.setattr(search, 'state_factored_search_device',
                        lambda agent, *a: calls.append(('device',) + a) or device_result)
    monkeypatch.setattr(frontier, 'state_factored_search', lambda agent, *a: calls.append(('host',) + a) or 'host result')
    return search, calls


def test_switch_defaults():
    from speaker_follower_amd import agents
    A = agents.Seq2SeqAgent
    assert A.search_on_device is False and A.search_fallbacks == 0 and A.device_search is None
    assert isinstance(A.search_chunk, int) and A.search_chunk >= 1


def test_switch_off_never_reaches_the_device_search(monkeypatch):
    search, calls = _patched(monkeypatch, 'device result')
    agent = _FakeAgent()
    agent.search_on_device = False
    assert search.state_factored_search(agent, 3, 1) == 'host result'
    assert [c[0] for c in calls] == ['host'] and agent.search_fallbacks == 0


def test_switch_on_runs_the_device_search(monkeypatch):
    search, calls = _patched(monkeypatch, 'device result')
    agent = _FakeAgent()
    assert search.state_factored_search(agent, 3, 1, False, True, 3) == 'device result'
    assert calls == [('device', 3, 1, False, True, 3)] and agent.search_fallbacks == 0


def test_an_overflow_runs_the_host_loop_over_the_same_minibatch(monkeypatch):
    search, calls = _patched(monkeypatch, None)
    agent = _FakeAgent()
    assert search.state_factored_search(agent, 3, 1, True, False, 4) == 'host result'
    assert calls == [('device', 3, 1, True, False, 4), ('host', 3, 1, False, False, 4)]   # (not the NEXT minibatch)
    assert agent.search_fallbacks == 1


@pytest.mark.parametrize('why', ['numpy', 'tie_log', 'decoder', 'successors', 'instances'])
def test_what_the_device_loop_does_not_take_runs_the_host_loop_and_is_counted(monkeypatch, why):
    search, calls = _patched(monkeypatch, 'device result', shape=(300, 6) if why == 'instances' else (8, 6))
    agent = _FakeAgent(visual=why != 'decoder')
    if why == 'numpy':
        agent.search_backend = 'numpy'
    if why == 'tie_log':
        agent.tie_log = []
    assert search.state_factored_search(agent, 3, 65 if why == 'successors' else 1) == 'host result'
    assert [c[0] for c in calls] == ['host'] and calls[0][3] is True                       # load_next_minibatch as given
    assert agent.search_fallbacks == 1


def test_graph_step_key_keeps_the_host_loop_keys_and_separates_the_device_loop():
    from speaker_follower_amd import search
    agent = type('A', (), {'decoder': object(), 'store': object()})()
    nav = object()
    host = search.graph_step_key(agent, nav, 8, 8, 80, 'fp32')
    assert host == (id(agent.decoder), id(agent.store), id(nav), 8, 8, 80) + search.gate_mode_key('fp32')
    dev = search.graph_step_key(agent, nav, 8, 8, 80, 'fp32', device_loop=(3, 1, 6, 4, 4, True, 2048, 1024))
    assert dev != host and dev[:len(host)] == host
    assert dev != search.graph_step_key(agent, nav, 8, 8, 80, 'fp32', device_loop=(3, 1, 6, 4, 8, True, 2048, 1024))
