"""GPU: sf_nav_follower_batches (csrc/sf_nav.hip) alone, through ctypes: every byte of `out`, col_route, col_len and err
== the numpy restatement of tests/follower_pack_cases.py (pinned to the host path by
tests/test_follower_routes_host.py); guard words around every output array, a fill pattern in the gaps between the
sections, between the blocks and behind the last one.

* B = 1, 2, 5, 63, 64, 65, 100 x Lmax = 1, 2, 8, 80 x M = 1, 3 (and 257 at Lmax = 8, and at B = 100, Lmax = 80) over routes of
  two scans with 5 and 9 hop rows under ld = 9 and 10; token counts 0, 1, Lmax - 2 .. Lmax + 1 and random ones, and no
  tokens at all; `reverse` on and off.
* all lengths equal (the draw order is kept), strictly increasing (fully reversed), ties at both ends, raw lengths
  above Lmax (equal after the cut, still sorted by raw length); a route drawn twice in one minibatch.
* the per-slot errors (route index -1 and N, view0 -1 and V, hop_rows > ld, a last token == eos) and every refusal of
  the entry (a misaligned `out` among them), with nothing written."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import follower_pack_cases as F                                     # noqa: E402

DEV = torch.device('cuda', 0)
GUARD, TAIL, FILL = -77, 8, 0x5A
V = 4
PAD, EOS = F.PAD, F.EOS


def guarded(n):
    return torch.full((TAIL + n + TAIL,), GUARD, dtype=torch.int32, device=DEV)


def plan(B, Lmax, ld, M, gap=64, tail=192):
    """(mb_off, total bytes): blocks `gap` bytes apart and `tail` bytes behind the last."""
    nbytes = F.layout(B, Lmax, ld)['bytes']
    return np.arange(M, dtype=np.int64) * (nbytes + gap), M * (nbytes + gap) + tail


def launch(rt, order, B, Lmax, ld, mb_off, total, tokens=None, instr_off=None, reverse=True, null=(), cols=True,
           mb_off_dev=None, fields=None, out_shift=0):
    """One raw launch.  Returns (status, outputs as host arrays, or None after a refusal -- when nothing may have been
    written, which is checked here, like the guard words)."""
    from speaker_follower_amd import _lib
    from speaker_follower_amd.runtime import stream
    N, M = len(rt['row0']), len(order) // B
    i32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)    # noqa: E731
    i64 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)    # noqa: E731
    ins = {k: i32(rt[k]) for k in ('row0', 'view0', 'hop_all', 'hop_base', 'hop_rows')}
    ins.update(hop_off=i64(rt['hop_off']), order=i32(order), instr_tokens=i64(tokens), instr_off=i64(instr_off))
    off_h = np.ascontiguousarray(mb_off, np.int64)
    ins['mb_off_dev'] = i64(off_h if mb_off_dev is None else mb_off_dev)
    bufs = dict(err=guarded(1), col_route=guarded(M * B), col_len=guarded(M * B),
                out=torch.full((TAIL + total + TAIL,), FILL, dtype=torch.uint8, device=DEV))
    bufs['err'][TAIL] = 0
    p = lambda x: None if x is None else x.data_ptr()               # noqa: E731
    f = dict(N=N, V=V, B=B, Lmax=Lmax, ld=ld, M=M, pad=PAD, eos=EOS, reverse=int(reverse), mb_off=off_h.ctypes.data,
             out=p(bufs['out'][TAIL + out_shift:]), out_bytes=total)
    f.update({k: p(v) for k, v in ins.items()})
    if cols:
        f.update(col_route=p(bufs['col_route'][TAIL:]), col_len=p(bufs['col_len'][TAIL:]))
    for k in null:
        if k not in ('io', 'err'):
            f[k] = None
    f.update(fields or {})                                          # (the struct's own sizes, overridden)
    io = _lib.NavFollowerIO(**f)
    status = _lib.lib.sf_nav_follower_batches(None if 'io' in null else C.byref(io),
                                              None if 'err' in null else C.c_void_p(p(bufs['err'][TAIL:])), stream())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, v in host.items():
        g = FILL if k == 'out' else GUARD
        assert (v[:TAIL] == g).all() and (v[-TAIL:] == g).all(), 'guard words of %s' % k
    if status != 0:
        assert (host['out'] == FILL).all() and host['err'][TAIL] == 0
        assert (host['col_route'] == GUARD).all() and (host['col_len'] == GUARD).all()
        return status, None
    if not cols:
        assert (host['col_route'] == GUARD).all() and (host['col_len'] == GUARD).all()
    return status, dict(out=host['out'][TAIL:-TAIL], err=int(host['err'][TAIL]),
                        col_route=host['col_route'][TAIL:-TAIL].reshape(M, B), col_len=host['col_len'][TAIL:-TAIL].reshape(M, B))


def check(rt, order, B, Lmax, ld, tokens=None, instr_off=None, reverse=True, cols=True, gap=64):
    """Launch == restatement, byte for byte (the gap bytes too: the restatement leaves them as they were)."""
    order = np.asarray(order, np.int32)
    mb_off, total = plan(B, Lmax, ld, len(order) // B, gap=gap)
    status, got = launch(rt, order, B, Lmax, ld, mb_off, total, tokens, instr_off, reverse, cols=cols)
    assert status == 0
    want = F.mirror_follower(rt, order, B, Lmax, ld, V, mb_off, np.full(total, FILL, np.uint8), tokens, instr_off, reverse)
    bad = np.flatnonzero(got['out'] != want['out'])
    assert len(bad) == 0, ('byte', int(bad[0]), 'of', len(bad), 'differ')
    free = F.gap_mask(B, Lmax, ld, mb_off, total)
    assert (got['out'][free] == FILL).all() and free[-192:].all() and free.sum() >= 192 + gap * (len(order) // B)
    assert got['err'] == want['err']
    if cols:
        assert (got['col_route'] == want['col_route']).all() and (got['col_len'] == want['col_len']).all()
    return got


def edge_lengths(rng, N, Lmax):
    """Token counts 0, 1, Lmax - 2 .. Lmax + 1 (each several times: ties) among random ones."""
    edges = [n for n in (0, 1, Lmax - 2, Lmax - 1, Lmax, Lmax + 1) if n >= 0]
    lens = rng.integers(0, Lmax + 4, N)
    at = rng.permutation(N)[:min(N, 3 * len(edges))]
    lens[at] = np.resize(edges, len(at))
    return lens


@pytest.mark.parametrize('B', [1, 2, 5, 63, 64, 65, 100])
def test_every_batch_size_width_and_minibatch_count(B):
    rng = np.random.default_rng(B)
    N = 150
    rt = F.random_routes(rng, N, scan_rows=(5, 9), V=V)
    for Lmax in (1, 2, 8, 80):
        tokens, off = F.tokens_of(rng, edge_lengths(rng, N, Lmax))
        for M in (1, 3, 257) if Lmax == 8 or (B, Lmax) == (100, 80) else (1, 3):
            order = rng.integers(0, N, M * B)
            ld = 9 + (M == 3)                                          # the largest scan, and one above it
            got = check(rt, order, B, Lmax, ld, tokens, off, reverse=bool((Lmax + M) & 2), gap=64 * (M % 3))
            assert got['err'] == 0 and got['col_len'].min() >= 1 and got['col_len'].max() <= Lmax
            sec = F.sections(got['out'][:F.layout(B, Lmax, ld)['bytes']], B, Lmax, ld)
            short = rt['hop_rows'][got['col_route'][0]] == 5
            assert (sec['hop'][short][:, 5:] == 0).all() and (sec['hop'][:, :5] > 0).all()     # zeros behind the shorter scan
            assert (sec['hop'][~short][:, :9] > 0).all() and (sec['hop'][:, 9:] == 0).all()
    check(rt, rng.integers(0, N, 2 * B), B, 8, 9, None, None, cols=False)   # no tokens at all, and no col arrays
    got = check(rt, rng.integers(0, N, 2 * B), B, 3, 9, None, None)
    assert (F.sections(got['out'][:F.layout(B, 3, 9)['bytes']], B, 3, 9)['seq'] == [EOS, PAD, PAD]).all()
    assert (got['col_len'] == 1).all()


def with_lengths(lens, seed=0):
    rng = np.random.default_rng(seed)
    rt = F.random_routes(rng, len(lens), scan_rows=(5, 9), V=V)
    tokens, off = F.tokens_of(rng, lens)
    return rt, tokens, off


@pytest.mark.parametrize('reverse', [True, False])
def test_length_patterns_decide_the_columns(reverse):
    B, Lmax = 6, 5
    # all equal: the draw order is kept
    rt, tokens, off = with_lengths([3] * B)
    draw = [4, 0, 5, 1, 3, 2]
    got = check(rt, draw, B, Lmax, 9, tokens, off, reverse)
    assert got['col_route'][0].tolist() == draw and got['col_len'][0].tolist() == [4] * B
    # strictly increasing: fully reversed
    rt, tokens, off = with_lengths([0, 1, 2, 3, 4, 5])
    got = check(rt, np.arange(B), B, Lmax, 9, tokens, off, reverse)
    assert got['col_route'][0].tolist() == [5, 4, 3, 2, 1, 0] and got['col_len'][0].tolist() == [5, 5, 4, 3, 2, 1]
    # ties at both ends
    rt, tokens, off = with_lengths([1, 4, 1, 4, 2, 1])
    got = check(rt, np.arange(B), B, Lmax, 9, tokens, off, reverse)
    assert got['col_route'][0].tolist() == [1, 3, 4, 0, 2, 5]
    # above Lmax: equal after the cut, still sorted by raw length; the cut keeps the front of what is stored
    rt, tokens, off = with_lengths([5, 9, 7, 4, 9, 6])
    got = check(rt, np.arange(B), B, Lmax, 9, tokens, off, reverse)
    assert got['col_route'][0].tolist() == [1, 4, 2, 5, 0, 3] and got['col_len'][0].tolist() == [5] * B
    seq = F.sections(got['out'][:F.layout(B, Lmax, 9)['bytes']], B, Lmax, 9)['seq']
    first = tokens[off[1]:off[2]]
    assert seq[0].tolist() == (first[::-1][:5] if reverse else first[:5]).tolist()
    assert seq[5].tolist() == (tokens[off[3]:off[4]][::-1] if reverse else tokens[off[3]:off[4]]).tolist() + [EOS]
    # a route drawn twice (and thrice) in one minibatch, over two minibatches
    got = check(rt, [2, 2, 0, 3, 2, 0, 1, 1, 1, 1, 1, 1], B, Lmax, 10, tokens, off, reverse)
    assert got['col_route'].tolist() == [[2, 2, 2, 0, 0, 3], [1] * 6]
    # a token that IS the pad id is masked like padding
    tokens2 = tokens.copy()
    tokens2[off[1] + 2] = PAD
    got = check(rt, np.arange(B), B, 12, 9, tokens2, off, reverse)
    sec = F.sections(got['out'][:F.layout(B, 12, 9)['bytes']], B, 12, 9)
    assert sec['mask'][0].sum() == 12 - 10 + 1 and (sec['mask'] == (sec['seq'] == PAD)).all()


def test_per_slot_errors_leave_an_empty_instruction():
    B, Lmax, ld = 5, 6, 9
    rt, tokens, off = with_lengths([3, 4, 2, 5, 1, 3, 2], seed=3)
    N = 7
    rt['hop_rows'][:] = [5, 9, 5, 9, 9, 5, 9]
    clean = check(rt, [0, 1, 2, 3, 4], B, Lmax, ld, tokens, off)
    assert clean['err'] == 0

    def column_of(got, r):
        c = got['col_route'][0].tolist().index(r)
        sec = F.sections(got['out'][:F.layout(B, Lmax, ld)['bytes']], B, Lmax, ld)
        return c, {k: v[c] for k, v in sec.items()}
    for r in (-1, N):                                                  # a route index outside the set: everything zero
        got = check(rt, [0, 1, r, 3, 4], B, Lmax, ld, tokens, off)
        c, col = column_of(got, r)
        assert got['err'] == 1 and c == B - 1 and col['seq'].tolist() == [EOS] + [PAD] * 5 and col['lengths'] == 1
        assert col['rows'] == 0 and col['views'] == 0 and col['base'] == 0 and (col['hop'] == 0).all()
        assert got['col_len'][0, c] == 1 and col['mask'].tolist() == [0] + [1] * 5
    for bad_view in (-1, V):
        rt2 = dict(rt, view0=rt['view0'].copy())
        rt2['view0'][3] = bad_view
        got = check(rt2, [0, 1, 2, 3, 4], B, Lmax, ld, tokens, off)
        c, col = column_of(got, 3)
        assert got['err'] == 1 and c == B - 1 and col['seq'].tolist() == [EOS] + [PAD] * 5 and col['lengths'] == 1
        assert col['rows'] == rt['row0'][3] and col['views'] == bad_view and col['base'] == rt['hop_base'][3]
    got = check(rt, [0, 1, 2, 3, 4], B, Lmax, 8, tokens, off)          # hop_rows 9 > ld 8 for routes 1, 3, 4
    assert got['err'] == 1 and got['col_route'][0].tolist() == [0, 2, 1, 3, 4] and got['col_len'][0].tolist() == [4, 3, 1, 1, 1]
    tokens2 = tokens.copy()
    tokens2[off[2] - 1] = EOS                                          # route 1 ends in eos
    tokens2[off[3]] = EOS                                              # route 3 holds one in front: fine
    got = check(rt, [0, 1, 2, 3, 4], B, Lmax, ld, tokens2, off)
    c, col = column_of(got, 1)
    assert got['err'] == 1 and c == B - 1 and col['seq'].tolist() == [EOS] + [PAD] * 5
    assert got['col_route'][0].tolist() == [3, 0, 2, 4, 1] and col['rows'] == rt['row0'][1] and (col['hop'] > 0).all()
    # a block the device copy of mb_off puts out of bounds is left alone, and raises err
    mb_off, total = plan(B, Lmax, ld, 2)
    status, got = launch(rt, np.array([0, 1, 2, 3, 4, 4, 3, 2, 1, 0], np.int32), B, Lmax, ld, mb_off, total, tokens, off,
                         mb_off_dev=np.array([mb_off[0], total], np.int64))
    nbytes = F.layout(B, Lmax, ld)['bytes']
    assert status == 0 and got['err'] == 1 and (got['out'][nbytes:] == FILL).all()
    assert (got['out'][:nbytes] == clean['out'][:nbytes]).all()


def test_entry_refusals_write_nothing():
    from speaker_follower_amd import _lib
    B, Lmax, ld = 3, 4, 9
    rt, tokens, off = with_lengths([3, 4, 2, 5], seed=4)
    order = np.array([0, 1, 2, 3, 2, 1], np.int32)
    mb_off, total = plan(B, Lmax, ld, 2)
    args = (rt, order, B, Lmax, ld, mb_off, total, tokens, off)
    assert launch(*args)[0] == 0
    ARG = (_lib.SF_ERR_ARG, None)
    for name in ('io', 'err', 'row0', 'view0', 'hop_all', 'hop_off', 'hop_base', 'hop_rows', 'order', 'mb_off', 'mb_off_dev',
                 'out', 'instr_tokens', 'instr_off', 'col_route', 'col_len'):
        assert launch(*args, null=(name,)) == ARG, name
    for field in ('N', 'V', 'B', 'Lmax', 'ld', 'M'):
        assert launch(*args, fields={field: 0}) == ARG, field
        assert launch(*args, fields={field: -1}) == ARG, field
    nbytes = F.layout(B, Lmax, ld)['bytes']
    for bad in ([0, -64], [0, nbytes + 8], [32, nbytes + 64], [0, total - nbytes + 64]):
        assert launch(rt, order, B, Lmax, ld, np.array(bad, np.int64), total, tokens, off) == ARG, bad
    assert launch(*args, fields=dict(out_bytes=int(mb_off[1]) + nbytes - 1)) == ARG
    for shift in (1, 4):                                               # `out` must be 8-byte aligned
        assert launch(*args, out_shift=shift) == ARG, shift
    assert launch(*args, fields=dict(out_bytes=int(mb_off[1]) + nbytes))[0] == 0
    # the cap: B = max_b runs, max_b + 1 is refused
    cap = _lib.lib.sf_nav_follower_batches_max_b()
    assert cap >= 1024
    rng = np.random.default_rng(9)
    for Bc, want in ((cap, 0), (cap + 1, _lib.SF_ERR_UNSUPPORTED)):
        order = rng.integers(0, 4, Bc).astype(np.int32)
        mb, tot = plan(Bc, 3, ld, 1)
        if want:
            assert launch(rt, order, Bc, 3, ld, mb, tot, tokens, off) == (want, None)
        else:
            check(rt, order, Bc, 3, ld, tokens, off)
