"""GPU: sf_nav_walk (csrc/sf_nav.hip) alone on hand-made tables, through ctypes: every element of its four outputs and
the error word == the numpy mirror of tests/nav_walk_cases.py (pinned to the host-path agents and through them to the
reference by tests/test_baseline_agents_host.py), with sentinels around every array.

* B = 1, 3, 4, 5 (around the four episodes of a block) and 257; S = 1, 2, 6, 7, 20; A = 1, 2, 16, 64 on random tables,
  the three policies; A = 65 refused.
* SHORTEST: goal = start, one hop, S - 1 / S / S + 1 hops (n_steps = min(k, S - 1) on both sides), a hop row that points
  at itself, two candidates to the hop, the hop only behind a_num, candidates that are the current row, two scans with
  their own hop_base under one ld_hop.
* RANDOM: first_action 1 and a_num - 1, 0 and a_num (refused per row), a dead end at moves 1 and 4, S = 5 refused.
* every SF_ERR_ARG with nothing written; view0 = -1 and V.
* the walk's arrays, unchanged, through sf_eval_score_routes == the same routes in the ragged layout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nav_walk_cases as W                                          # noqa: E402

DEV = torch.device('cuda', 0)
GUARD, TAIL = -77, 8
OUTS = ('row', 'view', 'actions', 'n_steps')


def guarded(n, dtype):
    return torch.full((TAIL + n + TAIL,), GUARD, dtype=dtype, device=DEV)


def launch(tab, policy, S, row0, view0, first=None, hop=None, base=None, B=None, null=(), ld_hop=None, table_null=(),
           A=None, V=None):
    """One raw launch.  Returns (status, outputs as host arrays -- err as an int -- or None when nothing may have been
    written); the guard words around every output are checked here, and after a refusal the outputs themselves."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import stream
    B = len(row0) if B is None else B
    n = max(len(row0), 1)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)   # noqa: E731
    t = {k: up(tab[k]) for k in ('a_num', 'next_row', 'cand_view')}
    ins = dict(row0=up(row0), view0=up(view0), first=up(first), hop=up(hop), base=up(base))
    S1 = max(S, 1)
    bufs = dict(row=guarded((S1 + 1) * n, torch.int32), view=guarded((S1 + 1) * n, torch.int32),
                actions=guarded(S1 * n, torch.int64), n_steps=guarded(n, torch.int32), err=guarded(1, torch.int32))
    bufs['err'][TAIL] = 0
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    tp = lambda k: None if k in table_null else t[k].data_ptr()     # noqa: E731
    nav = _lib.NavTableS(tp('a_num'), tp('next_row'), tp('cand_view'), None, None, tab['A'] if A is None else A,
                         tab['V'] if V is None else V)
    out_p = {k: None if k in null else p(v[TAIL:]) for k, v in bufs.items()}
    in_p = {k: None if k in null else p(v) for k, v in ins.items()}
    if ld_hop is None:
        ld_hop = hop.shape[1] if hop is not None else 0
    status = _lib.lib.sf_nav_walk(None if 'nav' in null else C.byref(nav), policy, B, S, in_p['row0'], in_p['view0'],
                                  in_p['first'], in_p['hop'], ld_hop, in_p['base'], out_p['row'], out_p['view'],
                                  out_p['actions'], out_p['n_steps'], out_p['err'], stream())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, v in host.items():
        assert (v[:TAIL] == GUARD).all() and (v[-TAIL:] == GUARD).all(), 'guard words of %s' % k
    if status != 0:
        for k in OUTS:
            assert (host[k] == GUARD).all(), '%s written by a refused call' % k
        assert host['err'][TAIL] == 0
        return status, None
    return status, dict(row=host['row'][TAIL:-TAIL].reshape(S + 1, n), view=host['view'][TAIL:-TAIL].reshape(S + 1, n),
                        actions=host['actions'][TAIL:-TAIL].reshape(S, n), n_steps=host['n_steps'][TAIL:-TAIL],
                        err=int(host['err'][TAIL]))


def check(tab, policy, S, row0, view0, first=None, hop=None, base=None):
    """Launch == mirror, element for element; returns the outputs."""
    status, got = launch(tab, policy, S, row0, view0, first, hop, base)
    assert status == 0
    want = W.mirror_walk(tab, policy, S, row0, view0, first, hop, base)
    for k in OUTS:
        assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), (k, got[k], want[k])
    assert got['err'] == want['err']
    return got


@pytest.mark.parametrize('policy', [W.STOP, W.SHORTEST, W.RANDOM])
@pytest.mark.parametrize('A', [1, 2, 16, 64])
def test_random_tables_at_every_batch_and_step_count(A, policy):
    rng = np.random.default_rng(1000 * A + policy)
    n_rows, V = 11, 3
    tab = W.random_table(rng, n_rows, V, A)
    for B in (1, 3, 4, 5, 257):
        for S in (1, 2, 6, 7, 20):
            if policy == W.RANDOM and S < W.RANDOM_MOVES + 1:
                continue
            row0 = rng.integers(0, n_rows, B).astype(np.int32)
            view0 = rng.integers(0, V, B).astype(np.int32)
            first = rng.integers(0, A + 2, B).astype(np.int32) if policy == W.RANDOM else None    # (0 and A + 1 among them)
            hop = W.random_hops(rng, tab, B, n_rows + 2) if policy == W.SHORTEST else None
            base = np.zeros(B, np.int32) if policy == W.SHORTEST else None
            got = check(tab, policy, S, row0, view0, first, hop, base)
            if policy == W.STOP:
                assert (got['n_steps'] == 0).all() and (got['row'] == row0).all() and (got['view'] == view0).all()
            if policy == W.RANDOM:
                assert set(got['n_steps'].tolist()) <= {-1, W.RANDOM_MOVES}
                if A >= 16 and B == 257:
                    assert got['err'] == 1 and len(set(got['n_steps'].tolist())) == 2      # refused rows beside walked ones


def test_more_than_64_candidate_slots_are_refused_with_nothing_written():
    from speaker_follower_amd import _lib
    tab = W.random_table(np.random.default_rng(65), 3, 2, 65)
    status, got = launch(tab, W.STOP, 2, np.zeros(3, np.int32), np.zeros(3, np.int32))
    assert status == _lib.SF_ERR_UNSUPPORTED and got is None


@pytest.mark.parametrize('S', [1, 2, 6, 7, 20])
def test_shortest_on_a_line(S):
    """Goals 0, 1, S - 1, S and S + 1 hops up the line: k = the hops where the stop still fits, else S; n_steps =
    min(k, S - 1).  Every state also has a candidate that is the current row, behind the real ones."""
    n_rows, V = S + 3, 2
    tab = W.line_table(n_rows, V, 4, extra=1)
    hops_away = [0, 1, max(S - 1, 0), S, S + 1]
    row0 = np.array([1] * len(hops_away), np.int32)
    view0 = np.array([0, 1, 0, 1, 0], np.int32)
    goals = [1 + d for d in hops_away]
    got = check(tab, W.SHORTEST, S, row0, view0, None, W.line_hops(n_rows, goals), np.zeros(len(goals), np.int32))
    assert got['n_steps'].tolist() == [min(d if d < S else S, S - 1) for d in hops_away]
    assert got['err'] == 0
    for b, d in enumerate(hops_away):                                 # the last pose of the result: as far as S - 1 moves get
        assert got['row'][got['n_steps'][b], b] == 1 + min(d, S - 1)
    # downwards too, in the same launch as a walk upwards
    got = check(tab, W.SHORTEST, S, np.array([S + 1, 0], np.int32), np.array([1, 1], np.int32), None,
                W.line_hops(n_rows, [0, 2]), np.zeros(2, np.int32))
    assert got['row'][-1].tolist() == [1, min(2, S)]


def test_shortest_teacher_rules():
    # rows 0 .. 5, V = 2; from (0, 0): slots 1 and 2 both lead to row 1 (views 1 and 0), slot 3 to row 2;
    # from (3, 0): one real candidate (row 4) and, BEHIND a_num, a slot that names row 5
    tab = W.make_table(6, 2, 8, {(0, 0): [(1, 1), (1, 0), (2, 1)], (1, 1): [(2, 0)], (3, 0): [(4, 0)], (2, 0): [(2, 1), (0, 0)]},
                       filler={(3, 0): [(5, 1)]})
    hop = np.array([[1, 2, 2, 3, 4, 5],          # two candidates lead to the hop: the first wins (arrives in view 1)
                    [0, 1, 2, 5, 4, 5],          # the hop of row 3 (row 5) exists only behind a_num: not taken, stop
                    [0, 1, 0, 3, 4, 5],          # from row 2: slot 1 is row 2 itself, slot 2 leads to the hop 0
                    [4, 1, 2, 3, 4, 5]], np.int32)   # the hop of row 0 is row 4: no candidate leads there, stop
    row0, view0 = np.array([0, 3, 2, 0], np.int32), np.zeros(4, np.int32)
    got = check(tab, W.SHORTEST, 6, row0, view0, None, hop, np.zeros(4, np.int32))
    assert got['actions'][:3, 0].tolist() == [1, 1, 0] and got['view'][1, 0] == 1 and got['n_steps'][0] == 2
    assert got['actions'][0, 1] == 0 and got['n_steps'][1] == 0 and (got['row'][:, 1] == 3).all()
    assert got['actions'][:2, 2].tolist() == [2, 0] and got['row'][1, 2] == 0
    assert got['actions'][0, 3] == 0 and got['n_steps'][3] == 0
    # a hop row that points at itself away from the goal: stops at once
    hop = np.array([[0, 1, 2, 3, 4, 5]], np.int32)
    got = check(tab, W.SHORTEST, 6, np.array([0], np.int32), np.array([0], np.int32), None, hop, np.zeros(1, np.int32))
    assert got['n_steps'][0] == 0 and (got['actions'] == 0).all() and (got['row'] == 0).all()


def test_shortest_rows_of_two_scans_in_one_launch():
    """Scan a = rows 0 .. 4, scan b = rows 5 .. 11: each row of the batch reads ITS hop row at row - hop_base, under one
    ld_hop larger than either scan."""
    a, b = W.line_table(5, 2, 3), W.line_table(7, 2, 3)
    nr_b = b['next_row'] + 5
    tab = dict(a_num=np.concatenate([a['a_num'], b['a_num']]), next_row=np.concatenate([a['next_row'], nr_b]),
               cand_view=np.concatenate([a['cand_view'], b['cand_view']]), A=3, V=2, n_rows=12)
    ld = 9
    hop = np.full((5, ld), -5, np.int32)
    goals = [(0, 4), (1, 6), (0, 0), (1, 0), (1, 3)]                  # (scan, local goal)
    for i, (s, g) in enumerate(goals):
        m, base = (5, 0) if s == 0 else (7, 5)
        hop[i, :m] = W.line_hops(m, [g], base=base)[0]
    base = np.array([0 if s == 0 else 5 for s, _ in goals], np.int32)
    row0 = np.array([0, 5, 3, 11, 8], np.int32)
    got = check(tab, W.SHORTEST, 8, row0, np.zeros(5, np.int32), None, hop, base)
    assert got['row'][-1].tolist() == [4, 11, 0, 5, 8] and got['n_steps'].tolist() == [4, 6, 3, 6, 0]


def chain_table(n_rows, A=4):
    """0 -> 1 -> .. -> n_rows - 1 by slot 1 (slot 2 leads back, slot 3 is the row itself); the last row is a dead end."""
    cands = {(r, v): [(r + 1, 1), (max(r - 1, 0), 0), (r, 1)] for r in range(n_rows - 1) for v in (0, 1)}
    return W.make_table(n_rows, 2, A, cands)


def test_random_first_actions_and_dead_ends():
    tab = chain_table(8)
    #            first = 1   a_num - 1 (itself)   0        a_num     dead end at move 1   at move 4   at the stop only
    row0 = np.array([0,          0,                0,       0,        6,                   3,          2], np.int32)
    first = np.array([1,         3,                0,       4,        1,                   1,          1], np.int32)
    view0 = np.zeros(len(row0), np.int32)
    for S in (6, 7, 20):
        got = check(tab, W.RANDOM, S, row0, view0, first)
        assert got['n_steps'].tolist() == [5, 5, -1, -1, -1, -1, 5] and got['err'] == 1
        assert got['actions'][:6, 0].tolist() == [1, 1, 1, 1, 1, 0] and got['row'][:6, 0].tolist() == [0, 1, 2, 3, 4, 5]
        assert got['row'][:3, 1].tolist() == [0, 0, 1] and got['view'][1, 1] == 0        # (a candidate that is the row: stays)
        for b in (2, 3, 4, 5):                                        # refused: actions 0, the start state throughout
            assert (got['actions'][:, b] == 0).all() and (got['row'][:, b] == row0[b]).all() and (got['view'][:, b] == 0).all()
        assert got['row'][5, 6] == 7 and (got['row'][5:, 6] == 7).all()
    # a launch without a refused row leaves the error word alone
    got = check(tab, W.RANDOM, 6, row0[[0, 1, 6]], view0[:3], first[[0, 1, 6]])
    assert got['err'] == 0


def test_start_views_outside_the_table_raise_the_error_word():
    tab = W.line_table(6, 3, 3)
    row0, view0 = np.array([1, 2, 3, 1, 1], np.int32), np.array([0, -1, 3, 2, 1], np.int32)
    for policy, S, first in ((W.STOP, 1, None), (W.SHORTEST, 4, None), (W.RANDOM, 6, np.ones(5, np.int32))):
        hop = W.line_hops(6, [4] * 5) if policy == W.SHORTEST else None
        base = np.zeros(5, np.int32) if policy == W.SHORTEST else None
        got = check(tab, policy, S, row0, view0, first, hop, base)
        assert got['err'] == 1 and got['n_steps'][1] == -1 == got['n_steps'][2] and (got['n_steps'][[0, 3, 4]] >= 0).all()
        assert (got['view'][:, 1] == -1).all() and (got['view'][:, 2] == 3).all() and (got['actions'][:, 1:3] == 0).all()


def test_every_argument_refusal_writes_nothing():
    from speaker_follower_amd import _lib
    tab = W.line_table(6, 2, 3)
    B = 3
    row0, view0, first = np.zeros(B, np.int32), np.zeros(B, np.int32), np.ones(B, np.int32)
    hop, base = W.line_hops(6, [3] * B), np.zeros(B, np.int32)
    ok = dict(tab=tab, policy=W.SHORTEST, S=6, row0=row0, view0=view0, first=first, hop=hop, base=base)
    assert launch(**ok)[0] == 0
    bad = [dict(null=(k,)) for k in ('nav', 'row0', 'view0', 'row', 'view', 'actions', 'n_steps', 'err')]
    bad += [dict(table_null=(k,)) for k in ('a_num', 'next_row', 'cand_view')]
    bad += [dict(B=0), dict(B=-1), dict(S=0), dict(S=-3), dict(A=0), dict(V=0), dict(policy=3), dict(policy=-1),
            dict(policy=W.RANDOM_MOVES), dict(null=('hop',)), dict(null=('base',)), dict(ld_hop=0),
            dict(policy=W.RANDOM, null=('first',)), dict(policy=W.RANDOM, S=5), dict(policy=W.RANDOM, S=1)]
    for change in bad:
        status, got = launch(**dict(ok, **change))
        assert status == _lib.SF_ERR_ARG and got is None, change
    # what a policy does not read may be missing
    assert launch(**dict(ok, policy=W.STOP, null=('first', 'hop', 'base'), ld_hop=0))[0] == 0
    assert launch(**dict(ok, policy=W.RANDOM, null=('hop', 'base'), ld_hop=0))[0] == 0
    assert launch(**dict(ok, null=('first',)))[0] == 0


def score_routes(D, m, B, n_slots, row, row_first, stride, n_steps, actions, S, gold_off, gold_node):
    """sf_eval_score_routes over one scan with table D [m, m], route b against gold path b; the eight outputs."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import stream
    up = lambda a, dt: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)    # noqa: E731
    i32, i64 = (lambda a: up(a, np.int32)), (lambda a: up(a, np.int64))                                       # noqa: E731
    t = dict(row=i32(row), first=i64(row_first), n=i32(n_steps), act=i64(actions), off=i32(gold_off), node=i32(gold_node),
             gid=i32(np.arange(B)), base=i32(np.zeros(B)), m=i32(np.full(B, m)), doff=i64(np.zeros(B)),
             slot=i32(np.arange(B)), D=torch.from_numpy(D).to(DEV))
    o64 = torch.full((5, n_slots), -7.25, dtype=torch.float64, device=DEV)
    o32 = torch.full((3, n_slots), -9, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda x: x.data_ptr()                                      # noqa: E731
    e = _lib.EvalRoutes(S, B, n_slots, stride, B, len(gold_node), int(np.diff(gold_off).max()), 0, t['row'].numel(),
                        p(t['row']), p(t['first']), p(t['n']), p(t['act']), p(t['off']), p(t['node']), p(t['gid']),
                        p(t['base']), p(t['m']), p(t['doff']), p(t['slot']), p(t['D']), 3.0,
                        *[p(o64[k]) for k in range(5)], *[p(o32[k]) for k in range(3)])
    _lib.call('sf_eval_score_routes', C.byref(e), C.c_void_p(p(err)), stream())
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    return o64.cpu().numpy(), o32.cpu().numpy()


def test_the_walk_arrays_feed_the_route_scorer_unchanged():
    """row [S+1,B] with row_stride = B, row_first[b] = b and the walk's n_steps == the same routes back to back."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import stream
    n_rows, S = 12, 7
    tab = W.line_table(n_rows, 2, 4, extra=1)
    D = (1.25 * np.abs(np.arange(n_rows)[:, None] - np.arange(n_rows)[None, :])).astype(np.float64)
    row0 = np.array([0, 2, 11, 5, 3], np.int32)
    goals = [4, 2, 1, 11, 0]
    B = len(goals)
    want = W.mirror_walk(tab, W.SHORTEST, S, row0, np.zeros(B, np.int32), None, W.line_hops(n_rows, goals), np.zeros(B, np.int32))
    assert want['n_steps'].tolist() == [4, 0, 6, 6, 3]
    gold = [list(range(r, g + 1)) if g >= r else list(range(r, g - 1, -1)) for r, g in zip(row0.tolist(), goals)]
    gold_off, gold_node = np.cumsum([0] + [len(g) for g in gold]), np.concatenate(gold)
    # the walk on the device, its tensors handed on as they are
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)      # noqa: E731
    t = [up(tab[k]) for k in ('a_num', 'next_row', 'cand_view')] + [up(row0), up(np.zeros(B)), up(W.line_hops(n_rows, goals)), up(np.zeros(B))]
    row, view = (torch.empty(S + 1, B, dtype=torch.int32, device=DEV) for _ in range(2))
    actions, n_steps = torch.empty(S, B, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())                          # noqa: E731
    nav = _lib.NavTableS(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, None, 4, 2)
    _lib.call('sf_nav_walk', C.byref(nav), W.SHORTEST, B, S, p(t[3]), p(t[4]), None, p(t[5]), n_rows, p(t[6]), p(row), p(view),
              p(actions), p(n_steps), p(err), stream())
    assert (row.cpu().numpy() == want['row']).all() and (n_steps.cpu().numpy() == want['n_steps']).all()
    sweep = score_routes(D, n_rows, B, B + 2, row, np.arange(B), B, n_steps, actions, S, gold_off, gold_node)
    poses = [want['row'][:n + 1, b] for b, n in enumerate(want['n_steps'].tolist())]
    ragged = score_routes(D, n_rows, B, B + 2, np.concatenate(poses), np.cumsum([0] + [len(x) for x in poses[:-1]]), 1,
                          want['n_steps'], np.zeros((1, B), np.int64), 1, gold_off, gold_node)
    for a, b in zip(sweep, ragged):
        assert (a == b).all()
    assert sweep[1][0, :B].tolist() == want['n_steps'].tolist()                     # steps
    assert sweep[0][0, :B].tolist() == [0.0, 0.0, 1.25 * 4, 1.25 * 0, 0.0]          # nav_error: walk 2 was cut off 4 rows short
    assert (sweep[0][:, B:] == -7.25).all() and (sweep[1][:, B:] == -9).all()
