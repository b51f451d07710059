"""Shared by tests/test_coverage_metrics_host.py and tests/test_gpu_coverage_metrics.py (no tests of its own): CLS
(coverage weighted by length score, Jain et al. 2019) restated in plain Python over a distance block and LOCAL node
lists, and the case list both files score.  The graphs and the eleven earlier values come from path_metric_cases.

    P = p_0 .. p_n the visited nodes, R = r_0 .. r_{g-1} the gold path, D[src][dst] the scan's distances, margin 3.0
    near[b]      = min over a of D[p_a][r_b]                        FROM the pose TO the gold node
    gold_length  = D[r_0][r_1] + D[r_1][r_2] + ...                  left to right; 0.0 for g == 1
    coverage     = (exp(-near[0] / margin) + ... + exp(-near[g-1] / margin)) / g     math.exp, left to right, inf -> 0.0
    expected     = coverage * gold_length
    length_score = 1.0 if expected + |expected - length| == 0, 0.0 if gold_length is inf,
                   else expected / (expected + |expected - length|)
    cls          = coverage * length_score

A minimum is exact, so the kernel's `near` must have these bits whatever order it folds in; everything after it is ONE
host function for the host and the device path: the tests compare with ==."""
import math

import numpy as np

import path_metric_cases as PM

MARGIN = PM.MARGIN
FIELDS = PM.FIELDS + ('gold_length', 'coverage', 'length_score', 'cls')
COVERAGE_LISTS = ('gold_lengths', 'coverage', 'length_score', 'cls')


def near_of(D, P, R, transposed=False):
    out = []
    for r in R:
        best = math.inf
        for p in P:
            d = float(D[r][p]) if transposed else float(D[p][r])
            if d < best:
                best = d
        out.append(best)
    return out


def gold_length_of(D, R):
    length = 0.0
    for u, v in zip(R[:-1], R[1:]):
        length = length + float(D[u][v])
    return length


def coverage_of(near, margin=MARGIN):
    total = 0.0
    for d in near:
        if d == math.inf:
            term = 0.0
        else:
            term = math.exp(-d / margin)
        total = total + term
    return total / len(near)


def four_of(near, gold_length, length, margin=MARGIN):
    """(gold_length, coverage, length_score, cls) from the three quantities they are functions of."""
    coverage = coverage_of(near, margin)
    expected = coverage * gold_length
    if gold_length == math.inf:
        length_score = 0.0
    elif expected + abs(expected - length) == 0:
        length_score = 1.0
    else:
        length_score = expected / (expected + abs(expected - length))
    return gold_length, coverage, length_score, coverage * length_score


def restate(D, P, R, margin=MARGIN):
    """The fifteen values of one result, in FIELDS order."""
    eleven = PM.restate(D, P, R, margin)
    return eleven + four_of(near_of(D, P, R), gold_length_of(D, R), eleven[3], margin)


# the issue's hand-checked rows on the unit line graph: (R, P, coverage, length_score, cls)
_C = (1.0 + math.exp(-1.0 / 3.0) + math.exp(-2.0 / 3.0) + math.exp(-1.0)) / 4
KNOWN = [([0, 1, 2, 3], [0, 1, 2, 3], 1.0, 1.0, 1.0),
         ([0, 1, 2, 3], [0], _C, 0.5, _C / 2),
         ([0, 1, 2, 3], [0, 1, 2, 3, 2, 3, 2, 3], 1.0, 3.0 / 7.0, 3.0 / 7.0),
         ([0], [0], 1.0, 1.0, 1.0),
         ([0], [0, 1], 1.0, 0.0, 0.0)]

GOLDS, POSES = (1, 2, 63, 64), (1, 2, 8, 9, 64, 65, 130)
N_CASES = 257
SIZES = {'a_single': 1, 'b_line6': 6, 'c_order': 4, 'd_two_parts': 12, 'e_rand70': 70, 'f_grid9': 9}

# apart from the case list (every gold path of which lies in one component): gold nodes no pose can reach -- an inf in
# `near`, a gold path of infinite length
UNREACHABLE = [('d_two_parts', [0, 1, 2], [0, 7, 8]),
               ('d_two_parts', [0, 1], [0, 1, 9]),
               ('d_two_parts', [6, 7, 8, 7], [6, 2])]


def cases():
    """[(scan, P, R)] with P[0] == R[0], local node indices: the hand-checked rows, a scan of one node, the direction of
    the distance, a pose in the other component (inf costs, every `near` finite), unit-weight ties, every gold length of
    GOLDS with every route length of POSES, then random routes up to N_CASES."""
    rng = np.random.default_rng(29)
    walk = lambda m, k, start: [start] + [int(x) for x in rng.integers(m, size=k - 1)]    # noqa: E731
    out = [('b_line6', P, R) for R, P, _, _, _ in KNOWN]
    out += [('a_single', [0], [0]),
            ('a_single', [0, 0, 0], [0]),
            ('c_order', [0], [0, 3]),                                 # D[0][3] = (.1 + .2) + .3 != D[3][0] = (.3 + .2) + .1
            ('c_order', [0, 1, 0], [0, 3]),
            ('c_order', [3, 0], [3, 2, 1, 0]),
            ('d_two_parts', [0, 7, 1], [0, 1, 2]),                    # a pose nobody can walk to: length inf, cls 0.0
            ('d_two_parts', [8, 3, 9], [8, 9, 10, 11]),
            ('f_grid9', [0, 1, 4, 5, 8], [0, 3, 4, 7, 8]),            # unit grid: several poses equally near
            ('f_grid9', [0, 3, 6, 7, 8, 5, 2, 1, 0], [0, 4, 8]),
            ('b_line6', [2, 2, 2], [2, 3, 4, 5])]
    for g in GOLDS:
        for k in POSES:
            R = walk(70, g, int(rng.integers(70)))
            out.append(('e_rand70', walk(70, k, R[0]), R))
    names = sorted(set(SIZES) - {'a_single'})
    while len(out) < N_CASES:
        s = names[int(rng.integers(len(names)))]
        R = walk(SIZES[s], int(rng.integers(1, 9)), int(rng.integers(SIZES[s])))
        P = walk(SIZES[s], int(rng.integers(1, 12)), R[0])
        if s == 'd_two_parts':                                        # nodes 0-5 / 6-11: the gold path stays in its start's
            R = [r % 6 + 6 * (R[0] // 6) for r in R]                  # component (the poses need not)
        out.append((s, P, R))
    return out


def first_of(the_cases, g, k):
    """Index of the first case with a gold path of g nodes and a route of k poses."""
    return next(i for i, (_, P, R) in enumerate(the_cases) if len(R) == g and len(P) == k)
