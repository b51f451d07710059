"""GPU: sf_nav_routes (csrc/sf_nav.hip) alone, through ctypes: every output == the numpy mirror of
tests/nav_route_cases.py (pinned to the host path by tests/test_routes_host.py), guard words around every array, a
guard pattern in the alignment gaps of the blocks, between them and behind the last one.

* N = 1, 3, 4, 5, 257 (around the four routes of a block) x B = 1, 2, 5, 100 x S = 1, 2, 7, 10 x A = 1, 2, 16, 64 on
  random tables, lengths mode and pack mode (which must agree on n_actions, reached and rows); A = 65 refused.
* routes of 0, S - 1, S and S + 1 hops, a goal with no path, two candidates to the hop, the hop only behind a_num, a
  candidate that is the current row; two scans under their own hop_off / hop_base; N % B != 0 with the tail filled from
  the front; instructions of 0, 1, Lmax - 2 .. Lmax + 1 tokens and none at all; mb_Tp at and one above the longest route.
* the per-route refusals (mb_Tp one below the longest route, view0 = -1 and V, a start row outside its hop block, a
  route index outside the split) and every SF_ERR_ARG with nothing written.
* the routes of the eight fixture scans in their minibatches == the host pack (RouteSet.pack against
  pack_speaker_batch of _index_batch(gold_routes))."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nav_route_cases as R                                         # noqa: E402
import nav_walk_cases as W                                          # noqa: E402

DEV = torch.device('cuda', 0)
GUARD, TAIL, FILL = -77, 8, 0x5A
WALK = ('n_actions', 'reached', 'rows')


def guarded(n, dtype=torch.int32):
    return torch.full((TAIL + n + TAIL,), GUARD, dtype=dtype, device=DEV)


def launch(tab, S, rt, route=None, pack=None, null=(), table_null=(), walk_arrays=True, **override):
    """One raw launch.  rt: dict(row0, view0, goal, hop_all, hop_off, hop_base, hop_rows); pack: dict(B, Lmax, mb_Tp,
    mb_off, total[, tokens, instr_off, mb_Tp_dev, mb_off_dev]).  Returns (status, outputs as host arrays or None after
    a refusal, when nothing may have been written -- checked here, like the guard words)."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import stream
    N = len(rt['row0'])
    n_slots = len(route) if route is not None else N
    i32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)    # noqa: E731
    i64 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)    # noqa: E731
    t = {k: i32(tab[k]) for k in ('a_num', 'next_row', 'cand_view')}
    t['feat_row'] = i32(tab.get('feat_row'))
    t['sincos'] = None if tab.get('sincos') is None else torch.from_numpy(tab['sincos']).to(DEV)
    ins = {k: i32(rt[k]) for k in ('row0', 'view0', 'goal', 'hop_all', 'hop_base', 'hop_rows')}
    ins['hop_off'], ins['route'] = i64(rt['hop_off']), i32(route)
    bufs = dict(n_actions=guarded(n_slots), reached=guarded(n_slots), rows=guarded((S + 1) * n_slots if S > 0 else n_slots),
                err=guarded(1))
    bufs['err'][TAIL] = 0
    p = lambda x: None if x is None else x.data_ptr()               # noqa: E731
    f = dict(N=N, S=S, n_slots=n_slots, B=0, Lmax=0, M=0, pad=R.PAD, eos=R.EOS)
    f.update({k: None if k in null else p(v) for k, v in ins.items()})
    if walk_arrays:
        f.update({k: None if k in null else p(bufs[k][TAIL:]) for k in WALK})
    keep = []
    if pack is not None:
        out = torch.full((TAIL + pack['total'] + TAIL,), FILL, dtype=torch.uint8, device=DEV)
        bufs['out'] = out
        Tp_h, off_h = np.ascontiguousarray(pack['mb_Tp'], np.int32), np.ascontiguousarray(pack['mb_off'], np.int64)
        Tp_d, off_d = i32(pack.get('mb_Tp_dev', Tp_h)), i64(pack.get('mb_off_dev', off_h))
        tok, ioff = i64(pack.get('tokens')), i64(pack.get('instr_off'))
        keep += [Tp_h, off_h, Tp_d, off_d, tok, ioff]
        f.update(B=pack['B'], Lmax=pack['Lmax'], M=len(Tp_h), mb_Tp=Tp_h.ctypes.data, mb_off=off_h.ctypes.data,
                 mb_Tp_dev=p(Tp_d), mb_off_dev=p(off_d), instr_tokens=p(tok), instr_off=p(ioff), out=p(out[TAIL:]),
                 out_bytes=pack['total'])
        for k in ('mb_Tp', 'mb_off', 'mb_Tp_dev', 'mb_off_dev', 'instr_tokens', 'instr_off'):
            if k in null:
                f[k] = None
    A, V = override.pop('A_', tab['A']), override.pop('V_', tab['V'])      # (the table's own two sizes)
    f.update(override)
    io = _lib.NavRoutesIO(**f)
    tp = lambda k: None if k in table_null else p(t[k])             # noqa: E731
    nav = _lib.NavTableS(tp('a_num'), tp('next_row'), tp('cand_view'), tp('sincos'), tp('feat_row'), A, V)
    status = _lib.lib.sf_nav_routes(None if 'nav' in null else C.byref(nav), None if 'io' in null else C.byref(io),
                                    None if 'err' in null else C.c_void_p(p(bufs['err'][TAIL:])), stream())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, v in host.items():
        g = FILL if k == 'out' else GUARD
        assert (v[:TAIL] == g).all() and (v[-TAIL:] == g).all(), 'guard words of %s' % k
    if status != 0:
        for k in WALK:
            assert (host[k] == GUARD).all(), '%s written by a refused call' % k
        assert 'out' not in host or (host['out'] == FILL).all()
        assert host['err'][TAIL] == 0
        return status, None
    got = dict(n_actions=host['n_actions'][TAIL:-TAIL], reached=host['reached'][TAIL:-TAIL],
               rows=host['rows'][TAIL:-TAIL].reshape(S + 1, n_slots), err=int(host['err'][TAIL]))
    if pack is not None:
        got['out'] = host['out'][TAIL:-TAIL]
    return status, got


def mirror(tab, S, rt, route=None, pack=None):
    pk = None if pack is None else dict(pack, out=np.full(pack['total'], FILL, np.uint8))
    return R.mirror_routes(tab, S, rt['row0'], rt['view0'], rt['goal'], rt['hop_all'], rt['hop_off'], rt['hop_base'],
                           rt['hop_rows'], route=route, pack=pk)


def check(tab, S, rt, route=None, pack=None, walk_arrays=True):
    """Launch == mirror, element for element (the gap bytes too: the mirror leaves them as they were)."""
    status, got = launch(tab, S, rt, route, pack, walk_arrays=walk_arrays)
    assert status == 0
    want = mirror(tab, S, rt, route, pack)
    for k in WALK if walk_arrays else ():
        assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), (k, got[k], want[k])
    assert got['err'] == want['err']
    if pack is not None:
        bad = np.flatnonzero(got['out'] != want['out'])
        assert len(bad) == 0, ('byte', int(bad[0]), 'of', len(bad), 'differ')
    return got


def both_modes(tab, S, rt, B, Lmax, tokens=None, instr_off=None, extra_Tp=0, gap=0):
    """Lengths mode, then pack mode over the blocks RouteSet.pack would lay out (tail filled from the front); the two
    must agree on the walk's arrays.  Returns (lengths outputs, pack outputs, route, mb_Tp, mb_off)."""
    first = check(tab, S, rt)
    N = len(rt['row0'])
    M = -(-N // B)
    route = (np.arange(M * B) % N).astype(np.int32)
    Tp, off, total = R.plan_blocks(first['n_actions'], route, B, Lmax, extra_Tp=extra_Tp, gap=gap)
    Tp = np.minimum(Tp, S).astype(np.int32) if extra_Tp else Tp
    pack = dict(B=B, Lmax=Lmax, mb_Tp=Tp, mb_off=off, total=total + 24, tokens=tokens, instr_off=instr_off)
    got = check(tab, S, rt, route, pack)
    for k in ('n_actions', 'reached'):
        assert (got[k] == first[k][route]).all()
    assert (got['rows'] == first['rows'][:, route]).all()
    free = R.gap_mask(B, Lmax, Tp, off, total + 24)
    assert (got['out'][free] == FILL).all() and free[-24:].all()
    return first, got, route, Tp, off


def one_scan(tab, hop_block, row0, view0, goal):
    """Routes over a table that is ONE scan from nav row 0, hop_block [m goals, m rows]."""
    m = hop_block.shape[0]
    n = len(row0)
    return dict(row0=np.asarray(row0, np.int32), view0=np.asarray(view0, np.int32), goal=np.asarray(goal, np.int32),
                hop_all=hop_block.reshape(-1).astype(np.int32), hop_off=np.asarray(goal, np.int64) * m,
                hop_base=np.zeros(n, np.int32), hop_rows=np.full(n, m, np.int32))


@pytest.mark.parametrize('B', [1, 2, 5, 100])
@pytest.mark.parametrize('A', [1, 2, 16, 64])
def test_random_tables_at_every_split_batch_and_step_count(A, B):
    rng = np.random.default_rng(100 * A + B)
    n_rows, V, Lmax = 11, 3, 6
    tab = R.with_pack_tables(W.random_table(rng, n_rows, V, A), rng)
    hop = W.random_hops(rng, tab, n_rows, n_rows)
    ended = set()
    for N in (1, 3, 4, 5, 257):
        for S in (1, 2, 7, 10):
            rt = one_scan(tab, hop, rng.integers(0, n_rows, N), rng.integers(0, V, N), rng.integers(0, n_rows, N))
            lens = rng.integers(0, Lmax + 3, N)
            instr_off = np.concatenate(([0], np.cumsum(lens)))
            tokens = rng.integers(4, 1000, int(instr_off[-1]) + 1)
            first, got, route, Tp, off = both_modes(tab, S, rt, B, Lmax, tokens, instr_off)
            assert first['err'] == 0 and (first['n_actions'] >= 1).all() and (first['n_actions'] <= S).all()
            ended |= set(zip(first['n_actions'].tolist(), first['reached'].tolist()))
    if A >= 16:
        assert {r for _, r in ended} == {0, 1} and len({n for n, _ in ended}) >= 4      # walks of many lengths, ending both ways


def test_more_than_64_candidate_slots_are_refused_with_nothing_written():
    from speaker_follower_amd import _lib
    rng = np.random.default_rng(65)
    tab = R.with_pack_tables(W.random_table(rng, 3, 2, 65), rng)
    rt = one_scan(tab, W.random_hops(rng, tab, 3, 3), [0, 1, 2], [0, 0, 1], [1, 1, 0])
    assert launch(tab, 4, rt) == (_lib.SF_ERR_UNSUPPORTED, None)
    pack = dict(B=3, Lmax=4, mb_Tp=[4], mb_off=[0], total=R.layout(3, 4, 4)['bytes'])
    assert launch(tab, 4, rt, np.arange(3, dtype=np.int32), pack) == (_lib.SF_ERR_UNSUPPORTED, None)


def line_block(n_rows):
    return W.line_hops(n_rows, list(range(n_rows)))                 # [goal, row]


@pytest.mark.parametrize('S', [1, 2, 7, 10])
def test_routes_of_every_length_on_a_line(S):
    """Goals 0, S - 1, S and S + 1 hops up the line (n = hops + 1 where the stop still fits: the last two are cut off and
    not reached), and downwards; every state also has a candidate that is the current row behind the real ones."""
    n_rows, V = S + 3, 2
    rng = np.random.default_rng(S)
    tab = R.with_pack_tables(W.line_table(n_rows, V, 4, extra=1), rng)
    hops_away = [0, max(S - 1, 0), S, S + 1]
    rt = one_scan(tab, line_block(n_rows), [1] * 4 + [S + 1], [0, 1, 0, 1, 1], [1 + d for d in hops_away] + [0])
    first, got, route, Tp, off = both_modes(tab, S, rt, 3, 5)
    assert first['n_actions'].tolist() == [min(d + 1, S) for d in hops_away] + [S]
    assert first['reached'].tolist() == [int(d + 1 <= S) for d in hops_away] + [0]
    assert first['rows'][-1].tolist() == [1 + min(d, S) for d in hops_away] + [1]
    assert first['rows'][0].tolist() == [1, 1, 1, 1, S + 1]
    assert first['err'] == 0 and Tp.tolist() == [S, S]


def test_teacher_rules_and_the_sections_of_a_block():
    # the table of tests/test_gpu_nav_walk.py: from (0, 0) slots 1 and 2 both lead to row 1 (views 1 and 0), slot 3 to
    # row 2; from (3, 0) one real candidate (row 4) and, BEHIND a_num, a slot that names row 5; (2, 0): slot 1 is row 2 itself
    rng = np.random.default_rng(3)
    tab = R.with_pack_tables(W.make_table(6, 2, 8, {(0, 0): [(1, 1), (1, 0), (2, 1)], (1, 1): [(2, 0)], (3, 0): [(4, 0)],
                                                    (2, 0): [(2, 1), (0, 0)]}, filler={(3, 0): [(5, 1)]}), rng)
    hop = np.tile(np.arange(6, dtype=np.int32), (6, 1))             # [goal, row]: every row points at itself ...
    hop[2] = [1, 2, 2, 3, 4, 5]      # goal 2 from row 0: two candidates lead to the hop 1, the first wins (arrives in view 1)
    hop[5] = [0, 1, 2, 5, 4, 5]      # goal 5 from row 3: the hop exists only behind a_num: stop, not reached
    hop[0] = [0, 1, 0, 3, 4, 5]      # goal 0 from row 2: slot 1 is row 2 itself, slot 2 leads to the hop
    hop[4] = [4, 1, 2, 3, 4, 5]      # goal 4 from row 0: no candidate leads to the hop 4: stop, not reached
    hop[3] = [0, 1, 2, 3, 4, 5]      # goal 3 from row 0: hop == row away from the goal (no path): one stop, not reached
    rt = one_scan(tab, hop, [0, 3, 2, 0, 0, 1], [0, 0, 0, 0, 0, 1], [2, 5, 0, 4, 3, 1])
    first, got, route, Tp, off = both_modes(tab, 6, rt, 6, 4)
    assert first['n_actions'].tolist() == [3, 1, 2, 1, 1, 1] and first['reached'].tolist() == [1, 0, 1, 0, 0, 1]
    assert first['rows'][:3, 0].tolist() == [0, 1, 2] and first['rows'][:2, 2].tolist() == [2, 0] and Tp.tolist() == [3]
    lay = R.layout(6, 3, 4)
    sec = lambda k, dt, shape: got['out'][lay[k][0]:lay[k][0] + lay[k][1]].view(dt).reshape(shape)         # noqa: E731
    assert sec('act', np.int32, (3, 6))[:, 0].tolist() == [1, 1, 0] and sec('view', np.int32, (3, 6))[:, 0].tolist() == [0, 1, 0]
    assert sec('act_view', np.int32, (3, 6))[:, 0].tolist() == [1, 0, 0]
    assert sec('vp', np.int32, (3, 6))[:, 0].tolist() == tab['feat_row'][[0, 1, 2]].tolist()
    assert sec('vp', np.int32, (3, 6))[:, 1].tolist() == [tab['feat_row'][3], -1, -1]
    sc = sec('act_sincos', np.uint32, (3, 6, 4))
    assert (sc[0, 0] == tab['sincos'][0, 1].view(np.uint32)).all() and (sc[1, 0] == tab['sincos'][3, 1].view(np.uint32)).all()
    assert sc[2, 0].view(np.float32).tolist() == [0.0, 1.0, 0.0, 1.0] == sc[1, 1].view(np.float32).tolist()
    assert sec('path_mask', np.uint8, (6, 3)).tolist() == [[0, 0, 0], [0, 1, 1], [0, 0, 1], [0, 1, 1], [0, 1, 1], [0, 1, 1]]
    assert (sec('instr_seq', np.int64, (6, 4)) == [R.EOS, R.PAD, R.PAD, R.PAD]).all()      # no tokens: empty instructions


def two_scan_routes():
    """Scan a = rows 0 .. 4, scan b = rows 5 .. 11, each with its own block of the hop table."""
    a, b = W.line_table(5, 2, 3), W.line_table(7, 2, 3)
    tab = dict(a_num=np.concatenate([a['a_num'], b['a_num']]), next_row=np.concatenate([a['next_row'], b['next_row'] + 5]),
               cand_view=np.concatenate([a['cand_view'], b['cand_view']]), A=3, V=2, n_rows=12)
    hop_all = np.concatenate([line_block(5).reshape(-1), (line_block(7) + 5).reshape(-1)]).astype(np.int32)
    pairs = [(0, 0, 4), (1, 5, 11), (0, 3, 0), (1, 11, 5), (1, 8, 8), (0, 4, 2), (1, 6, 9)]        # (scan, start, goal)
    rt = dict(row0=np.array([p[1] for p in pairs], np.int32), view0=np.zeros(len(pairs), np.int32),
              goal=np.array([p[2] for p in pairs], np.int32), hop_all=hop_all,
              hop_off=np.array([(p[2] * 5) if p[0] == 0 else 25 + (p[2] - 5) * 7 for p in pairs], np.int64),
              hop_base=np.array([0 if p[0] == 0 else 5 for p in pairs], np.int32),
              hop_rows=np.array([5 if p[0] == 0 else 7 for p in pairs], np.int32))
    return tab, rt


def test_two_scans_and_a_ragged_tail_filled_from_the_front():
    tab, rt = two_scan_routes()
    tab = R.with_pack_tables(tab, np.random.default_rng(2))
    first, got, route, Tp, off = both_modes(tab, 8, rt, 3, 5, gap=16)
    assert first['n_actions'].tolist() == [5, 7, 4, 7, 1, 3, 4] and first['reached'].all() and first['err'] == 0
    assert route.tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1] and Tp.tolist() == [7, 7, 7]              # 7 routes in blocks of 3
    assert first['rows'][-1].tolist() == rt['goal'].tolist()


def test_instruction_lengths_and_block_step_counts():
    rng = np.random.default_rng(12)
    Lmax, S = 7, 6
    tab = R.with_pack_tables(W.line_table(9, 2, 3), rng)
    lens = [0, 1, Lmax - 2, Lmax - 1, Lmax, Lmax + 1]
    rt = one_scan(tab, line_block(9), [0] * 6, [0, 1] * 3, [1, 2, 3, 4, 2, 1])
    instr_off = np.concatenate(([0], np.cumsum(lens)))
    tokens = rng.integers(4, 1000, int(instr_off[-1]))
    for extra in (0, 1):                                              # Tp = the longest route of the minibatch, and one more
        first, got, route, Tp, off = both_modes(tab, S, rt, 6, Lmax, tokens, instr_off, extra_Tp=extra)
        assert Tp.tolist() == [5 + extra]
        seq = got['out'][:6 * Lmax * 8].view(np.int64).reshape(6, Lmax)
        assert (seq == R.EOS).sum(1).tolist() == [1, 1, 1, 1, 0, 0] and seq[0].tolist() == [R.EOS] + [R.PAD] * (Lmax - 1)
        assert seq[3].tolist() == tokens[instr_off[3]:instr_off[4]].tolist() + [R.EOS]
        assert seq[5].tolist() == tokens[instr_off[5]:instr_off[5] + Lmax].tolist()
    both_modes(tab, S, rt, 4, Lmax)                                   # no tokens at all, and a tail


def test_per_route_refusals_raise_the_error_word_and_disturb_nothing_else():
    rng = np.random.default_rng(5)
    tab = R.with_pack_tables(W.line_table(8, 3, 3), rng)
    blk = line_block(8)
    # a block one step short of its longest route: that route alone becomes one stop at its start
    rt = one_scan(tab, blk, [0, 1, 2, 0], [0, 1, 2, 0], [2, 5, 3, 0])
    first = check(tab, 6, rt)
    assert first['n_actions'].tolist() == [3, 5, 2, 1] and first['err'] == 0
    route = np.arange(4, dtype=np.int32)
    pack = dict(B=4, Lmax=3, mb_Tp=[4], mb_off=[0], total=R.layout(4, 4, 3)['bytes'] + 8)
    got = check(tab, 6, rt, route, pack)
    assert got['err'] == 1 and got['n_actions'].tolist() == [3, 5, 2, 1] and (got['rows'] == first['rows']).all()
    lay = R.layout(4, 4, 3)
    mask = got['out'][lay['path_mask'][0]:lay['path_mask'][0] + 16].reshape(4, 4)
    assert mask.tolist() == [[0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1]]
    # start views outside the table, a start row outside its hop block (before it and behind it), a route index outside
    rt = one_scan(tab, blk, [1, 2, 3, 7, 1, 1], [0, -1, 3, 0, 2, 1], [4, 4, 4, 4, 4, 4])
    rt['hop_base'][3], rt['hop_rows'][4] = 8, 1
    route = np.array([0, 1, 2, 3, 4, 5, 6, -1], np.int32)
    first = check(tab, 5, rt)
    assert first['err'] == 1 and first['n_actions'].tolist() == [4, 1, 1, 1, 1, 4] and first['reached'].tolist() == [1, 0, 0, 0, 0, 1]
    assert (first['rows'][:, 1:5] == [2, 3, 7, 1]).all()
    Tp, off, total = R.plan_blocks(first['n_actions'], route % 6, 4, 3)
    got = check(tab, 5, rt, route, dict(B=4, Lmax=3, mb_Tp=Tp, mb_off=off, total=total))
    assert got['err'] == 1 and got['n_actions'].tolist() == [4, 1, 1, 1, 1, 4, 1, 1] and (got['rows'][:, 6:] == 0).all()
    vp = got['out'][R.layout(4, 4, 3)['vp'][0]:][:64].view(np.int32).reshape(4, 4)
    assert vp[0].tolist() == [tab['feat_row'][1], tab['feat_row'][2], tab['feat_row'][3], -1]
    # a launch without a refused route leaves the error word alone
    assert check(tab, 5, one_scan(tab, blk, [1], [0], [4]))['err'] == 0


def test_every_argument_refusal_writes_nothing():
    from speaker_follower_amd import _lib
    tab = R.with_pack_tables(W.line_table(6, 2, 3), np.random.default_rng(1))
    rt = one_scan(tab, line_block(6), [0, 1, 2], [0, 0, 1], [3, 3, 5])
    route = np.arange(6, dtype=np.int32) % 3
    S, B, Lmax = 6, 2, 4
    size = R.layout(B, 4, Lmax)['bytes']
    pack = dict(B=B, Lmax=Lmax, mb_Tp=[4, 4, 4], mb_off=[0, size, 2 * size], total=3 * size)
    ok = dict(tab=tab, S=S, rt=rt)
    ok_pack = dict(ok, route=route, pack=pack)
    assert launch(**ok)[0] == 0 and launch(**ok_pack)[0] == 0
    walk_in = ('row0', 'view0', 'goal', 'hop_all', 'hop_off', 'hop_base', 'hop_rows')
    bad = [dict(null=(k,)) for k in ('nav', 'io', 'err') + walk_in + WALK]
    bad += [dict(table_null=(k,)) for k in ('a_num', 'next_row', 'cand_view')]
    bad += [dict(N=0), dict(N=-1), dict(S=0), dict(S=-2), dict(n_slots=0), dict(n_slots=-4), dict(A_=0), dict(V_=0)]
    for change in bad:
        assert launch(**dict(ok, **change)) == (_lib.SF_ERR_ARG, None), change
        if not set(change.get('null', ())) & set(WALK):
            assert launch(**dict(ok_pack, **change)) == (_lib.SF_ERR_ARG, None), change
    bad = [dict(null=(k,)) for k in ('mb_Tp', 'mb_off', 'mb_Tp_dev', 'mb_off_dev', 'instr_tokens', 'n_actions', 'reached', 'rows')]
    bad += [dict(table_null=(k,)) for k in ('sincos', 'feat_row')]
    bad += [dict(B=0), dict(B=-1), dict(Lmax=0), dict(Lmax=-1), dict(M=0), dict(M=2), dict(n_slots=5), dict(out_bytes=0),
            dict(out_bytes=3 * size - 1), dict(B=3)]
    bad += [dict(pack=dict(pack, mb_Tp=tp)) for tp in ([4, 0, 4], [4, 4, S + 1], [-1, 4, 4])]
    bad += [dict(pack=dict(pack, mb_off=o)) for o in ([0, size, 2 * size + 8], [0, size + 4, 2 * size], [-8, size, 2 * size])]
    tokens = dict(tokens=np.arange(10), instr_off=np.array([0, 2, 5, 9]))
    assert launch(**dict(ok_pack, pack=dict(pack, **tokens)))[0] == 0
    for change in bad:
        assert launch(**dict(ok_pack, pack=dict(change.pop('pack', pack), **tokens), **change)) == (_lib.SF_ERR_ARG, None), change
    # what a mode does not read may be missing: the walk's arrays in pack mode (all three), the tokens
    assert launch(**dict(ok_pack, walk_arrays=False))[0] == 0
    check(tab, S, rt, route, pack, walk_arrays=False)
    # device copies that are not what the entry checked: the kernel leaves those minibatches alone and raises err
    status, got = launch(**dict(ok_pack, pack=dict(pack, mb_Tp_dev=[4, S + 1, 4], mb_off_dev=[0, size, 2 * size + 8])))
    want = mirror(tab, S, rt, route, pack)
    assert status == 0 and got['err'] == 1 and (got['out'][:size] == want['out'][:size]).all() and (got['out'][size:] == FILL).all()


@pytest.fixture(scope='module')
def fixture_routes():
    from speaker_follower_amd.routes import RouteSet
    env, nav, dist, _ = R.fixture_world('cuda')
    rs = RouteSet.enumerate(nav, dist)
    return nav, rs, rs.items()


@pytest.mark.parametrize('B,chunk', [(100, None), (7, 50)])
def test_the_fixture_scans_routes_in_their_minibatches_equal_the_host_pack(fixture_routes, B, chunk):
    nav, rs, items = fixture_routes
    S, Lmax = 10, 12
    lens = rs.lengths(S)
    wn, wreached, wrows = rs.walk_host(S)
    assert (lens['n_actions'].cpu().numpy() == wn).all() and (lens['reached'].cpu().numpy() == 1).all()
    assert (lens['rows'].cpu().numpy() == wrows).all() and int(lens['err'].item()) == 0
    packed = rs.pack(B, Lmax, chunk=chunk, S=S)
    torch.cuda.synchronize()
    assert int(packed.err.item()) == 0 and len(packed) == -(-1734 // B) and (packed.n_actions == wn).all()
    assert len({id(b[0]) for b in packed.blocks}) == (1 if chunk is None else -(-len(packed) // chunk))
    want = R.host_blocks(nav, items, packed.route, B, Lmax, S)
    for i, (t, buf) in enumerate(want):
        assert packed.blocks[i][2] == t
        assert R.sections_equal(packed.block(i).cpu().numpy(), buf, B, t, Lmax) == [], i
