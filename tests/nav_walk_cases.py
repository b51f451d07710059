"""sf_nav_walk (include/sf_hip.h) restated in numpy, and small hand-made navigation tables to hold the kernel to.

`mirror_walk` is written from the entry's contract, not from the kernel: one Python loop per episode.  A table here is
a dict(a_num [n*V], next_row [n*V,A], cand_view [n*V,A], A, V, n_rows) of int32 arrays, state s = row * V + view."""
import numpy as np

STOP, SHORTEST, RANDOM, RANDOM_MOVES = 0, 1, 2, 5


def mirror_walk(tab, policy, S, row0, view0, first_action=None, goal_hop=None, hop_base=None):
    """dict(row, view [S+1,B] int32, actions [S,B] int64, n_steps [B] int32, err 0/1): what one launch leaves."""
    a_num, next_row, cand_view, A, V = (tab[k] for k in ('a_num', 'next_row', 'cand_view', 'A', 'V'))
    B = len(row0)
    row, view = np.zeros((S + 1, B), np.int32), np.zeros((S + 1, B), np.int32)
    actions, n_steps, err = np.zeros((S, B), np.int64), np.zeros(B, np.int32), 0
    for b in range(B):
        start = (int(row0[b]), int(view0[b]))
        r, v = start
        states, acts = [start], []
        bad = not 0 <= v < V
        while not bad and len(acts) < S:
            t, s = len(acts), r * V + v
            n = min(int(a_num[s]), A)
            a = 0
            if policy == SHORTEST:
                hop = int(goal_hop[b][r - int(hop_base[b])])
                if hop != r:
                    for c in range(1, n):
                        if next_row[s, c] == hop:
                            a = c
                            break
            elif policy == RANDOM:
                if t == 0:
                    a = int(first_action[b])
                    bad = not 1 <= a < n
                elif t < RANDOM_MOVES:
                    a = 1
                    bad = n <= 1
                if bad:
                    break
            if a >= n:                                       # (an action the state does not have counts as 0)
                a = 0
            if a != 0 and next_row[s, a] != r:               # a candidate that is the current row leaves the state
                r, v = int(next_row[s, a]), int(cand_view[s, a])
            acts.append(a)
            states.append((r, v))
            if a == 0:
                break
        if bad:
            err, n, states, acts = 1, -1, [start], []
        elif policy == SHORTEST:
            k = acts.index(0) if 0 in acts else S
            n = min(k, S - 1)
        else:
            n = 0 if policy == STOP else RANDOM_MOVES
        acts += [0] * (S - len(acts))                         # after the stop: action 0, the last state again
        states += [states[-1]] * (S + 1 - len(states))
        row[:, b], view[:, b] = [x[0] for x in states], [x[1] for x in states]
        actions[:, b], n_steps[b] = acts, n
    return dict(row=row, view=view, actions=actions, n_steps=n_steps, err=err)


def make_table(n_rows, V, A, cands, filler=None):
    """cands: (row, view) -> [(next_row, cand_view), ...] for slots 1, 2, ..; a state not named has the stop slot only.
    filler: (row, view) -> [(next_row, cand_view), ...] written from slot a_num on (what no walk may read as a
    candidate).  Every other slot holds the state's own row and view 0, as nav.NavTable pads."""
    a_num = np.ones(n_rows * V, np.int32)
    next_row = np.repeat(np.arange(n_rows, dtype=np.int32), V)[:, None].repeat(A, 1).copy()
    cand_view = np.zeros((n_rows * V, A), np.int32)
    for (r, v), lst in cands.items():
        s = r * V + v
        a_num[s] = 1 + len(lst)
        assert a_num[s] <= A
        for c, (nr, cv) in enumerate(lst, 1):
            next_row[s, c], cand_view[s, c] = nr, cv
    for (r, v), lst in (filler or {}).items():
        s = r * V + v
        for c, (nr, cv) in enumerate(lst, int(a_num[s])):
            next_row[s, c], cand_view[s, c] = nr, cv
    return dict(a_num=a_num, next_row=next_row, cand_view=cand_view, A=A, V=V, n_rows=n_rows)


def line_table(n_rows, V, A, extra=0):
    """Rows 0 .. n_rows-1 on a line.  In every view, slot 1 leads up (to row + 1, arriving in view (view + 1) % V), slot 2
    down (to row - 1, view 0) where there is one; `extra` further slots lead to the state's own row."""
    cands = {}
    for r in range(n_rows):
        for v in range(V):
            lst = []
            if r + 1 < n_rows:
                lst.append((r + 1, (v + 1) % V))
            if r > 0:
                lst.append((r - 1, 0))
            cands[(r, v)] = (lst + [(r, 0)] * extra)[:A - 1]
    return make_table(n_rows, V, A, cands)


def line_hops(n_rows, goals, base=0, ld=None):
    """hop [len(goals), ld] of the line: one row towards the goal, the goal itself at the goal."""
    hop = np.zeros((len(goals), ld or n_rows), np.int32)
    for b, g in enumerate(goals):
        for r in range(n_rows):
            hop[b, r] = base + r + (g > r) - (g < r)
    return hop


def random_table(rng, n_rows, V, A):
    """Any table at all: candidate counts 1 .. A, targets anywhere (the own row among them), views anywhere."""
    a_num = rng.integers(1, A + 1, n_rows * V).astype(np.int32)
    next_row = rng.integers(0, n_rows, (n_rows * V, A)).astype(np.int32)
    next_row[:, 0] = np.repeat(np.arange(n_rows), V)
    cand_view = rng.integers(0, V, (n_rows * V, A)).astype(np.int32)
    return dict(a_num=a_num, next_row=next_row, cand_view=cand_view, A=A, V=V, n_rows=n_rows)


def random_hops(rng, tab, B, ld):
    """hop rows over the whole table as one scan (hop_base = 0): an eighth point at the row itself (a stop), an eighth
    anywhere, the others at what some slot of some view of the row names -- mostly a candidate of the state the walk is
    in, sometimes one of another view or one behind a_num, so walks run on for a while and end in every way."""
    n, V, A = tab['n_rows'], tab['V'], tab['A']
    own = np.arange(ld, dtype=np.int64)[None, :].repeat(B, 0) % n
    named = tab['next_row'][own * V + rng.integers(0, V, (B, ld)), rng.integers(0, A, (B, ld))]
    u = rng.random((B, ld))
    return np.where(u < 1 / 8, own, np.where(u < 1 / 4, rng.integers(0, n, (B, ld)), named)).astype(np.int32)
