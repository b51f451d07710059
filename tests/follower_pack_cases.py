"""sf_nav_follower_batches (include/sf_hip.h) restated in numpy: one Python loop per minibatch, written from the entry's
contract, not from the kernel; the block layout restated; builders for random route and token sets over the tables of
tests/nav_walk_cases.py (the entry copies hop rows, it does not walk: any table serves)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nav_walk_cases as W                                          # noqa: E402

PAD, EOS = 0, 2
SECTIONS = ('seq', 'mask', 'lengths', 'rows', 'views', 'hop', 'base')


def layout(B, Lmax, ld):
    """nav.DeviceNavBatch.pack_layout restated: name -> (offset, bytes), and 'bytes'; every section on a 64-byte boundary."""
    off, lay = 0, {}
    for name, nbytes in zip(SECTIONS, (B * Lmax * 8, B * Lmax, B * 4, B * 4, B * 4, B * ld * 4, B * 4)):
        lay[name] = (off, nbytes)
        off = (off + nbytes + 63) // 64 * 64
    lay['bytes'] = off
    return lay


def sections(blk, B, Lmax, ld):
    """The seven sections of one block (a uint8 array) as typed views."""
    lay = layout(B, Lmax, ld)
    sec = lambda name, dt, shape: blk[lay[name][0]:lay[name][0] + lay[name][1]].view(dt).reshape(shape)   # noqa: E731
    return dict(seq=sec('seq', np.int64, (B, Lmax)), mask=sec('mask', np.uint8, (B, Lmax)), lengths=sec('lengths', np.int32, (B,)),
                rows=sec('rows', np.int32, (B,)), views=sec('views', np.int32, (B,)), hop=sec('hop', np.int32, (B, ld)),
                base=sec('base', np.int32, (B,)))


def gap_mask(B, Lmax, ld, mb_off, total):
    """bool [total]: True for every byte no section covers (the alignment gaps, between and behind the blocks)."""
    free = np.ones(total, bool)
    lay = layout(B, Lmax, ld)
    for off in mb_off:
        for name in SECTIONS:
            free[int(off) + lay[name][0]:int(off) + lay[name][0] + lay[name][1]] = False
    return free


def mirror_follower(rt, order, B, Lmax, ld, V, mb_off, out, tokens=None, instr_off=None, reverse=True, pad=PAD, eos=EOS):
    """dict(out, err, col_route, col_len): what one launch leaves.  rt: dict(row0, view0, hop_all, hop_off, hop_base,
    hop_rows); out: the uint8 buffer as it stands before the launch."""
    N, M = len(rt['row0']), len(order) // B
    out, err = out.copy(), 0
    col_route, col_len = np.zeros((M, B), np.int32), np.zeros((M, B), np.int32)
    for i in range(M):
        slots = []
        for r in (int(x) for x in order[i * B:(i + 1) * B]):
            known = 0 <= r < N
            toks = []
            if known and tokens is not None:
                toks = [int(x) for x in tokens[int(instr_off[r]):int(instr_off[r + 1])]]
            bad = (not known or not 0 <= int(rt['view0'][r]) < V or int(rt['hop_rows'][r]) > ld
                   or (len(toks) > 0 and toks[-1] == eos))
            if bad:
                err, toks = 1, []
            slots.append((r, known, toks))
        columns = sorted(range(B), key=lambda j: len(slots[j][2]), reverse=True)     # stable: equal lengths in draw order
        sec = sections(out[int(mb_off[i]):int(mb_off[i]) + layout(B, Lmax, ld)['bytes']], B, Lmax, ld)
        for c, j in enumerate(columns):
            r, known, toks = slots[j]
            row = ((toks[::-1] if reverse else toks) + [eos])[:Lmax]
            sec['seq'][c] = row + [pad] * (Lmax - len(row))
            sec['mask'][c] = sec['seq'][c] == pad
            sec['lengths'][c] = col_len[i, c] = min(len(toks) + 1, Lmax)
            col_route[i, c] = r
            sec['hop'][c] = 0
            if known:
                m = min(max(int(rt['hop_rows'][r]), 0), ld)
                sec['hop'][c, :m] = rt['hop_all'][int(rt['hop_off'][r]):int(rt['hop_off'][r]) + m]
            sec['rows'][c] = rt['row0'][r] if known else 0
            sec['views'][c] = rt['view0'][r] if known else 0
            sec['base'][c] = rt['hop_base'][r] if known else 0
    return dict(out=out, err=err, col_route=col_route, col_len=col_len)


def random_routes(rng, N, scan_rows=(5, 9), V=4, first_row=3):
    """N routes over scans of `scan_rows` rows laid out from nav row `first_row`: the arrays sf_nav_routes and
    sf_nav_follower_batches share.  Each scan's hop block [goal, row] is nav_walk_cases.random_hops over a random table."""
    n_rows = first_row + sum(scan_rows)
    tab = W.random_table(rng, n_rows, V, 3)
    base = first_row + np.concatenate(([0], np.cumsum(scan_rows)[:-1]))
    off = np.concatenate(([0], np.cumsum(np.square(scan_rows))[:-1]))
    hop_all = np.concatenate([1 + W.random_hops(rng, tab, m, m).reshape(-1) for m in scan_rows]).astype(np.int32)
    scan = rng.integers(0, len(scan_rows), N)
    m = np.asarray(scan_rows)[scan]
    goal = rng.integers(0, m)
    return dict(row0=(base[scan] + rng.integers(0, m)).astype(np.int32), view0=rng.integers(0, V, N).astype(np.int32),
                hop_all=hop_all, hop_off=(off[scan] + goal * m).astype(np.int64), hop_base=base[scan].astype(np.int32),
                hop_rows=m.astype(np.int32))


def tokens_of(rng, lens, lo=4, hi=1000):
    """(flat int64 ids in [lo, hi) with one spare element behind, instr_off [N+1] int64) for the given token counts."""
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return rng.integers(lo, hi, int(off[-1]) + 1).astype(np.int64), off


def encodings(tokens, instr_off):
    return [tokens[int(a):int(b)] for a, b in zip(instr_off[:-1], instr_off[1:])]
