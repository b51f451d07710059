"""sf_nav_routes (include/sf_hip.h) restated in numpy: one Python loop per slot, written from the entry's contract, not
from the kernel.  Tables are those of tests/nav_walk_cases.py (a dict of a_num, next_row, cand_view, A, V, n_rows), for
pack mode with `sincos` [n*V, A, 4] float32 and `feat_row` [n_rows] int32 beside them."""
import numpy as np

PAD, EOS = 0, 2


def layout(B, Tp, Lmax):
    """speaker.packed_layout restated: name -> (offset, bytes), and 'bytes'."""
    off, lay = 0, {}
    for name, nbytes in (('instr_seq', B * Lmax * 8), ('vp', Tp * B * 4), ('view', Tp * B * 4), ('act', Tp * B * 4),
                         ('act_view', Tp * B * 4), ('act_sincos', Tp * B * 16), ('path_mask', B * Tp)):
        lay[name] = (off, nbytes)
        off = (off + nbytes + 7) // 8 * 8
    lay['bytes'] = off
    return lay


def with_pack_tables(tab, rng):
    """The table with random float32 bit patterns as its sincos (finite ones: compared as integers anyway) and a
    permutation as its feature rows."""
    n, A, V = tab['n_rows'], tab['A'], tab['V']
    out = dict(tab)
    out['sincos'] = rng.standard_normal((n * V, A, 4)).astype(np.float32)
    out['feat_row'] = (rng.permutation(n) + 1000).astype(np.int32)
    return out


def walk(tab, S, row, view, hop_row, base, m):
    """The teacher's walk: (steps [(row, view, slot)], stopped, last row), or None where a row leaves the hop block."""
    a_num, next_row, cand_view, A, V = (tab[k] for k in ('a_num', 'next_row', 'cand_view', 'A', 'V'))
    steps, stopped = [], False
    while not stopped and len(steps) < S:
        if not 0 <= row - base < m:
            return None
        s = row * V + view
        hop, a = int(hop_row[row - base]), 0
        if hop != row:
            for c in range(1, min(int(a_num[s]), A)):
                if next_row[s, c] == hop:
                    a = c
                    break
        steps.append((row, view, a))
        if a != 0 and next_row[s, a] != row:
            row, view = int(next_row[s, a]), int(cand_view[s, a])
        stopped = a == 0
    return steps, stopped, row


def mirror_routes(tab, S, row0, view0, goal, hop_all, hop_off, hop_base, hop_rows, route=None, n_slots=None, pack=None):
    """dict(n_actions, reached [n_slots] int32, rows [S+1, n_slots] int32, err, out): what one launch leaves.  pack:
    dict(B, Lmax, mb_Tp, mb_off, out = the uint8 buffer as it stands before the launch, tokens, instr_off)."""
    N, V, A = len(row0), tab['V'], tab['A']
    n_slots = (len(route) if route is not None else N) if n_slots is None else n_slots
    n_actions, reached = np.zeros(n_slots, np.int32), np.zeros(n_slots, np.int32)
    rows, err = np.zeros((S + 1, n_slots), np.int32), 0
    out = None if pack is None else pack['out'].copy()
    for j in range(n_slots):
        r = int(route[j]) if route is not None else j
        known = 0 <= r < N
        start = (int(row0[r]), int(view0[r])) if known else (0, 0)
        base, m = (int(hop_base[r]), int(hop_rows[r])) if known else (0, 0)
        row_ok = known and 0 <= start[0] - base < m
        w = None
        if row_ok and 0 <= start[1] < V:
            w = walk(tab, S, start[0], start[1], hop_all[int(hop_off[r]):int(hop_off[r]) + m], base, m)
        if w is None:                                          # one stop at the start
            err = 1
            n_actions[j], reached[j], rows[:, j] = 1, 0, start[0]
            column = [(tab['feat_row'][start[0]] if row_ok else -1, start[1], 0)] if pack else None
        else:
            steps, stopped, last = w
            n_actions[j], reached[j] = len(steps), int(stopped and last == int(goal[r]))
            visited = [x[0] for x in steps] + [last]
            rows[:, j] = visited + [last] * (S + 1 - len(visited))
            column = steps
        if pack is None:
            continue
        B, Lmax = pack['B'], pack['Lmax']
        i, col = divmod(j, B)
        Tp, lay = int(pack['mb_Tp'][i]), layout(B, int(pack['mb_Tp'][i]), Lmax)
        blk = out[int(pack['mb_off'][i]):int(pack['mb_off'][i]) + lay['bytes']]
        sec = lambda name, dt, shape: blk[lay[name][0]:lay[name][0] + lay[name][1]].view(dt).reshape(shape)   # noqa: E731
        if w is not None and len(column) > Tp:                 # too long for its block: one stop at the start
            err = 1
            column = [(start[0], start[1], 0)]
        if w is not None:
            column = [(int(tab['feat_row'][x[0]]), x[1], x[2], x[0] * V + x[1]) for x in column]
        vp, view, act, act_view = (sec(k, np.int32, (Tp, B)) for k in ('vp', 'view', 'act', 'act_view'))
        sincos, mask = sec('act_sincos', np.uint32, (Tp, B, 4)), sec('path_mask', np.uint8, (B, Tp))
        stop_bits = np.array([0.0, 1.0, 0.0, 1.0], np.float32).view(np.uint32)
        for t in range(Tp):
            if t < len(column):
                a = column[t][2]
                vp[t, col], view[t, col], act[t, col] = column[t][0], column[t][1], int(a != 0)
                act_view[t, col] = tab['cand_view'][column[t][3], a] if a else 0
                sincos[t, col] = tab['sincos'][column[t][3], a].view(np.uint32) if a else stop_bits
                mask[col, t] = 0
            else:
                vp[t, col], view[t, col], act[t, col], act_view[t, col] = -1, 0, 0, 0
                sincos[t, col] = stop_bits
                mask[col, t] = 1
        toks = []
        if pack.get('tokens') is not None and known:
            toks = [int(x) for x in pack['tokens'][int(pack['instr_off'][r]):int(pack['instr_off'][r + 1])]]
        seq = sec('instr_seq', np.int64, (B, Lmax))
        seq[col] = PAD
        k = min(len(toks), Lmax - 1)
        seq[col, :k] = toks[:k]
        if len(toks) + 1 <= Lmax:
            seq[col, k] = EOS
        else:
            seq[col, Lmax - 1] = toks[Lmax - 1]
    return dict(n_actions=n_actions, reached=reached, rows=rows, err=err, out=out)


def plan_blocks(n_actions, route, B, Lmax, extra_Tp=0, gap=0):
    """(mb_Tp, mb_off, total bytes) the way RouteSet.pack lays a chunk out: Tp = the longest route of the minibatch
    (+ extra_Tp), blocks back to back (+ `gap` bytes, a multiple of 8, between them)."""
    M = len(route) // B
    Tp = n_actions[route].reshape(M, B).max(1).astype(np.int32) + extra_Tp
    size = np.array([layout(B, int(t), Lmax)['bytes'] + gap for t in Tp], np.int64)
    off = np.concatenate(([0], np.cumsum(size)))
    return Tp.astype(np.int32), off[:-1].astype(np.int64), int(off[-1])


def gap_mask(B, Lmax, mb_Tp, mb_off, total):
    """bool [total]: True for every byte no section covers (the alignment gaps, between and behind the blocks)."""
    free = np.ones(total, bool)
    for Tp, off in zip(mb_Tp, mb_off):
        lay = layout(B, int(Tp), Lmax)
        for name in lay:
            if name != 'bytes':
                free[int(off) + lay[name][0]:int(off) + lay[name][0] + lay[name][1]] = False
    return free


# ---- the eight committed connectivity graphs as a world, and the host path's bytes to hold the kernel to
def fixture_world(device='cpu'):
    """(env, nav table, distance table) over tests/golden/connectivity, every viewpoint a feature row."""
    import os
    import types
    import torch
    from speaker_follower_amd.build import build_sim
    build_sim(verbose=False)
    from speaker_follower_amd import env, evaluation, nav
    conn = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'connectivity')
    scans = sorted(open(os.path.join(conn, 'scans.txt')).read().split())
    graphs = {s: env.NavGraph(os.path.join(conn, s + '_connectivity.json')) for s in scans}
    row_of, n = {}, 0
    for s in scans:
        for v in graphs[s].ids:
            row_of[s + '_' + v] = n
            n += 1
    e = env.R2RIndexEnv([], row_of, conn, batch_size=100, scans=scans)
    table = nav.NavTable(e, types.SimpleNamespace(device=torch.device(device)))
    return e, table, evaluation.DistanceTable(e.graphs, device='cpu'), n


def table_of(nav_table):
    h = nav_table.host
    return dict(a_num=h['a_num'], next_row=h['next_row'], cand_view=h['cand_view'], sincos=h['sincos'],
                feat_row=h['feat_row'], A=h['next_row'].shape[1], V=36, n_rows=nav_table.n_rows)


def host_blocks(nav_table, items, route, B, Lmax, S):
    """Per minibatch (Tp, the bytes pack_speaker_batch writes for _index_batch(gold_routes(...)) of its items)."""
    from speaker_follower_amd import agents, speaker
    out = []
    for lo in range(0, len(route), B):
        mb = [items[r] for r in route[lo:lo + B]]
        n, rows = nav_table.gold_routes(mb, S)
        first = np.concatenate(([0], np.cumsum(n)))
        sb = agents.Seq2SeqSpeaker._index_batch(n, lambda a, b: rows[first[a]:first[b]], [it['instr_encoding'] for it in mb], 0, B)
        Tp = int(n.max())
        buf = np.full(layout(B, Tp, Lmax)['bytes'], 0xA5, np.uint8)
        speaker.pack_speaker_batch(sb, buf, Lmax)
        out.append((Tp, buf))
    return out


def sections_equal(a, b, B, Tp, Lmax):
    """The names of the sections in which two blocks differ (the gaps are not compared)."""
    lay = layout(B, Tp, Lmax)
    return [k for k in lay if k != 'bytes' and not (a[lay[k][0]:lay[k][0] + lay[k][1]] == b[lay[k][0]:lay[k][0] + lay[k][1]]).all()]
