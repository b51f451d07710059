"""The GEMM dispatch asked on the host: csrc/sf_gemm_plan.h decides which kernel forms a product -- pure C++ that includes no
HIP header -- and csrc/sf_gemm.hip only issues what a plan says.  tests/gemm_plan_shim.cpp wraps the plan functions; it is
compiled here with g++ and loaded with ctypes.  No GPU, no HIP, nothing of the library itself is loaded.

The plans are asked the way the entries ask them (csrc/sf_api.hip): sf_linear_fwd with one segment, the epilogue of `act`,
neither raw slabs nor ksplit_out; sf_linear_slabs_fwd with two segments, raw slabs and ksplit_out, packed weights only when
sf_gate_product_bf16_weights is on (it is off in the GPU tests); sf_linear_bwd as gemm_nn_ws(M, K, N) for dx, gemm_tn(M, N, K)
with ldy = lddy for dW and colsum(M, N) for db.  Each gets the 64 MiB workspace less its 2048 ticket words."""
import ctypes as C
import os
import subprocess

import pytest

from tests import gemm_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = (64 << 20) // 4 - 2048                       # floats the entries hand on: sf_workspace_bytes() / 4 - SYNC_WORDS
AMPLE = 1 << 40
OK, UNSUPPORTED, WORKSPACE = 0, 2, 4
NT_SMALL, NT_BF16W, NT_BIG, NT_SPLIT, NT_TILED, NT_STREAM = range(6)
TN_MANY_ROW, TN_SPLIT, TN_TILED, TN_STREAM, TN_COLUMN_CUT = range(5)
EPI_NONE, EPI_TANH, EPI_MUL, EPI_TANHBWD = range(4)
BF16W, SMALL_X = 'gemm_nt_bf16w_kernel<%d>', 'gemm_nt_small_x_kernel<%d, %d>'
i64 = C.c_longlong


class Job(C.Structure):
    _fields_ = [('M', C.c_int), ('P', C.c_int), ('Q', C.c_int), ('ldy', C.c_int), ('ldx', C.c_int), ('Y', i64), ('X', i64)]


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp('gemm_plan') / 'gemm_plan_shim.so'
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-shared', '-fPIC',
                    '-I' + os.path.join(ROOT, 'speaker_follower_amd', 'csrc'), os.path.join(ROOT, 'tests', 'gemm_plan_shim.cpp'),
                    '-o', str(so)], check=True)
    return Shim(C.CDLL(str(so)))


class Shim:
    def __init__(self, lib):
        self.lib = lib
        for f in (lib.shim_plan_nt, lib.shim_plan_nn, lib.shim_plan_tn, lib.shim_plan_colsum):
            f.restype = None
        # the switches as the library starts with them (csrc/sf_gemm.hip: g_nt_force_f32 ... g_tn_group)
        self.defaults = dict(f32=0, big=1, big_ksplit=1, tn_rows=4096, tn_group=1)
        t = (C.c_int * 64)()
        n = lib.shim_tables(t)
        self.small_insts = {(t[2 * i], t[2 * i + 1]) for i in range(10)}
        self.nt_mt_max = t[20]
        self.nn_insts = set(t[21:n])
        self._out = (i64 * 256)()

    def switches(self, **kw):
        assert set(kw) <= set(self.defaults)
        d = dict(self.defaults, **kw)
        if d['tn_rows'] < 0:
            d['tn_rows'] = self.defaults['tn_rows']            # sf_debug_tn_split_min_rows(-1): the default
        return (C.c_int * 5)(d['f32'], d['big'], d['big_ksplit'], d['tn_rows'], d['tn_group'])

    def nt(self, M, N, Ks, ws=WS, raw=0, ksplit_out=0, packed=0, epi=EPI_NONE, accumulate=0, addend=0, r1_s=0, **sw):
        Ks = (Ks,) if isinstance(Ks, int) else tuple(Ks)
        flags = (C.c_int * 7)(raw, ksplit_out, packed, epi, accumulate, addend, r1_s)
        self.lib.shim_plan_nt(M, N, (C.c_int * 3)(*Ks), len(Ks), flags, i64(ws), self.switches(**sw), self._out)
        keys = 'status family mt cpw extras gx gy gz block lds ksplit slabs reduce ws'.split()
        return dict(zip(keys, self._out[:14]))

    def nn(self, M, N, K, ws=WS):
        self.lib.shim_plan_nn(M, N, K, i64(ws), self._out)
        return dict(zip('mt mblocks ks gx gy gz ws sizing'.split(), self._out[:8]))

    def tn(self, M, P, Q, ldy=None, ws=WS, **sw):
        self.lib.shim_plan_tn(M, P, Q, P if ldy is None else ldy, i64(ws), self.switches(**sw), self._out)
        keys = 'family splits gx gy gz off_xt off_slabs ws'.split()
        part = lambda i: dict(zip(keys, self._out[8 * i:8 * i + 8]))
        p = part(0)
        p.update(main=part(1), tail=part(2), q_main=self._out[24], main_columns=self._out[25])
        return p

    def tn_group(self, jobs, ws=WS, **sw):
        arr = (Job * len(jobs))(*[Job(*j) for j in jobs])
        n = self.lib.shim_plan_tn_group(arr, len(jobs), i64(ws), self.switches(**sw), self._out)
        o = self._out[:n]
        g = dict(zip('grouped n ntr reduce most ws'.split(), o[:6]))
        g['jobs'] = [dict(zip('job ks yt xt off_slabs'.split(), o[6 + 5 * k:11 + 5 * k])) for k in range(g['n'])]
        g['tr'] = [dict(zip('job x off'.split(), o[46 + 3 * j:49 + 3 * j])) for j in range(g['ntr'])]
        return g

    def colsum(self, M, N, ws=WS):
        self.lib.shim_plan_colsum(M, N, i64(ws), self._out)
        return dict(zip('ms gx gy fx ws'.split(), self._out[:5]))


# ---------------------------------------------------------------------------- a plan as kernel names
def nt_launches(p):
    """The kernels (as kernel_profile() spells them) an OK plan of linear_nt launches."""
    assert p['status'] == OK, p
    name = {NT_SMALL: (SMALL_X if p['extras'] else G.SMALL) % (p['mt'], p['cpw']), NT_BF16W: BF16W % p['mt'], NT_BIG: G.BIG,
            NT_SPLIT: G.SPLIT % p['mt'], NT_TILED: G.TILED % p['mt'], NT_STREAM: G.NT % p['mt']}[p['family']]
    return {name, G.REDUCE} if p['reduce'] else {name}


def add(counts, name, n=1):
    counts[name] = counts.get(name, 0) + n


def tn_launches(p, counts):
    if p['family'] == TN_COLUMN_CUT:
        tn_launches(p['main'], counts)
        tn_launches(p['tail'], counts)
        return
    if p['family'] == TN_MANY_ROW:
        add(counts, G.TRANSPOSE, 2)
        add(counts, G.BIG)
    else:
        add(counts, {TN_SPLIT: G.TN_SPLIT, TN_TILED: G.TN_TILED, TN_STREAM: G.TN}[p['family']])
    if p['splits'] > 1:
        add(counts, G.REDUCE)


def bwd_launches(shim, M, N, K, with_dx, tn_rows, lddy):
    """Launch counts of sf_linear_bwd with act = 0, dW and db asked for: what it composes from the three plans."""
    counts = {}
    if with_dx:
        p = shim.nn(M, K, N)
        assert p['mt'] in shim.nn_insts
        add(counts, G.NN % p['mt'])
        add(counts, G.REDUCE, int(p['ks'] > 1))
    tn_launches(shim.tn(M, N, K, ldy=lddy, tn_rows=tn_rows), counts)
    p = shim.colsum(M, N)
    add(counts, G.COLSUM)
    add(counts, G.COLSUM_FINISH, int(p['ms'] > 1))
    return counts


# ------------------------------------------------------------------------- the tables of gemm_cases
def test_forward_cases_reach_the_kernels_they_name(shim):
    for c in G.FORWARD:
        for epi in (EPI_NONE, EPI_TANH):
            got = nt_launches(shim.nt(c.M, c.N, c.K, epi=epi, f32=c.f32))
            assert got == set(c.kernels), (c, epi, got)
            assert not got & set(c.absent), (c, epi, got)
    for c in G.DENSE:
        if c.entry == 'fwd':
            for epi in (EPI_NONE, EPI_TANH):
                assert c.kernel in nt_launches(shim.nt(c.M, c.N, c.K, epi=epi, f32=c.f32)), c


def test_slab_cases_reach_the_kernels_they_name(shim):
    for c in G.SLABS:
        p = shim.nt(c.M, c.N, (c.K1, c.K2), raw=1, ksplit_out=1)
        assert nt_launches(p) == set(c.kernels) and not p['reduce'], (c, p)
        assert p['ksplit'] > 1 and p['slabs'] and p['ws'] == p['ksplit'] * c.M * c.N, (c, p)


def test_backward_cases_launch_what_they_count(shim):
    cases = [(dict(c.kernels), c.M, c.N, c.K, c.with_dx, c.tn_split_min_rows) for c in G.BACKWARD]
    cases += [({c.kernel: 1}, c.M, c.N, c.K, True, c.tn_split_min_rows) for c in G.DENSE if c.entry == 'bwd']
    assert len(cases) == len(G.BACKWARD) + 5
    for want, M, N, K, with_dx, rows in cases:
        for lddy in (N, N + 4, N + 12):                       # the row strides of dy the GPU module uses
            got = bwd_launches(shim, M, N, K, with_dx, rows, lddy)
            for name, n in want.items():
                assert got.get(name, 0) == n, ((M, N, K, lddy), name, n, got)
    # spelled out: the column cut is two gemm_tn_kernel launches and ONE slab sum; the many-row form two transposes and
    # gemm_nt_big_kernel, with the slab sum of its 8 K splits
    cut = bwd_launches(shim, 512, 2048, 4352, False, -1, 2048)
    assert cut == {G.TN: 2, G.REDUCE: 1, G.COLSUM: 1, G.COLSUM_FINISH: 1}, cut
    many = bwd_launches(shim, 1024, 64, 64, False, -1, 64)
    assert many == {G.TRANSPOSE: 2, G.BIG: 1, G.REDUCE: 1, G.COLSUM: 1, G.COLSUM_FINISH: 1}, many


# ------------------------------------------------------------------------------------ thresholds
def test_many_row_kernel_thresholds(shim):
    fam = lambda *a, **k: shim.nt(*a, **k)['family']
    assert fam(512, 64, 2320) == NT_BIG and fam(511, 64, 2320) != NT_BIG
    assert fam(512, 64, 2320) == NT_BIG and fam(512, 63, 2320) != NT_BIG
    assert fam(512, 2048, 52) == NT_BIG and fam(512, 2048, 48) != NT_BIG            # four chunks of 16
    assert fam(512, 64, (2320, 32)) == NT_BIG and fam(512, 64, (2320, 28)) != NT_BIG   # every segment NB_K deep
    assert fam(512, 64, 2320, epi=EPI_TANH) == NT_BIG and fam(512, 64, 2320, epi=EPI_MUL) != NT_BIG
    assert fam(512, 64, 2320, accumulate=1) == NT_BIG and fam(512, 64, 2320, epi=EPI_TANH, accumulate=1) != NT_BIG
    assert fam(512, 64, 2320, addend=1) == NT_BIG and shim.nt(512, 64, 2320, r1_s=1)['status'] == UNSUPPORTED
    assert fam(512, 64, 2320, big=0) == NT_STREAM
    # K splits: raw slabs, ksplit_out and the switch bit, all three; 2 560 x 2 048 (320 tiles) takes 3
    beam = dict(raw=1, ksplit_out=1, ws=AMPLE)
    assert shim.nt(2560, 2048, 2368, **beam)['ksplit'] == 3
    assert shim.nt(2560, 2048, 2368, raw=1, ws=AMPLE)['ksplit'] == 1
    assert shim.nt(2560, 2048, 2368, ksplit_out=1)['ksplit'] == 1
    assert shim.nt(2560, 2048, 2368, big_ksplit=0, **beam)['ksplit'] == 1
    assert shim.nt(2560, 2048, 32 * 48, **beam)['ksplit'] == 3 and shim.nt(2560, 2048, 32 * 47, **beam)['ksplit'] == 2
    assert shim.nt(2560, 2048, 32 * 32, **beam)['ksplit'] == 2 and shim.nt(2560, 2048, 32 * 31, **beam)['ksplit'] == 1
    mn = 2560 * 2048
    assert shim.nt(2560, 2048, 2368, raw=1, ksplit_out=1, ws=3 * mn - 1)['ksplit'] == 2
    assert shim.nt(2560, 2048, 2368, raw=1, ksplit_out=1, ws=2 * mn - 1)['ksplit'] == 1
    assert shim.nt(2560, 2048, 2368, raw=1, ksplit_out=1, ws=mn - 1)['family'] != NT_BIG


def test_split_and_tiled_thresholds(shim):
    # raw slabs keep the short-reduction kernel out of the way.  One block of rows, 128 chunks, N % 64, every K % 64:
    # a depth of 127 chunks is not a multiple of 64, so the nearest depths that differ in the chunk count alone are 124 / 128
    for f32, family in ((0, NT_SPLIT), (1, NT_TILED)):
        fam = lambda M, N, K: shim.nt(M, N, K, raw=1, f32=f32)['family']
        assert fam(100, 128, 2048) == family and fam(100, 128, 1984) == NT_STREAM
        assert fam(100, 128, 2032) == NT_STREAM                                      # 127 chunks (and K % 64 != 0)
        assert fam(100, 128, (2048, 64)) == family and fam(100, 128, (2048, 48)) == NT_STREAM
        assert fam(100, 192, 2048) == family and fam(100, 132, 2048) == NT_STREAM
    assert shim.nt(128, 128, 2368)['family'] == NT_SPLIT and shim.nt(129, 128, 2368)['family'] == NT_STREAM   # one row block
    assert shim.nt(128, 128, 2368, f32=1)['family'] == NT_TILED and shim.nt(129, 128, 2368, f32=1)['family'] == NT_STREAM
    # unsplit and unreduced, the epilogue must be none: K = 2048 over [16, 2048 * 64] has one K split
    assert shim.nt(16, 131072, 2048, epi=EPI_NONE)['ksplit'] == 1
    assert shim.nt(16, 131072, 2048, epi=EPI_NONE)['family'] == NT_SPLIT
    assert shim.nt(16, 131072, 2048, epi=EPI_TANH)['family'] == NT_STREAM
    # the cap of the row-block rule: ceil(N / 64) ks <= 256 when there is one row block and 128 chunks
    p = shim.nt(100, 2176, 2048)
    assert (p['family'], p['ksplit'], p['gx'] * p['gy']) == (NT_SPLIT, 7, 34 * 7)
    assert shim.nt(100, 2176, 2032)['ksplit'] == 8                                   # not tiled-eligible by depth: no cap
    # bf16-stored weights: packed weights, raw slabs, M <= 128, every K % 64; MT = ceil(M / 16); no degrade
    bw = dict(raw=1, ksplit_out=1, packed=1)
    for M in (1, 16, 17, 128):
        p = shim.nt(M, 2048, (2368, 512), **bw)
        assert (p['family'], p['mt'], p['status']) == (NT_BF16W, (M + 15) // 16, OK), p
        assert p['lds'] == shim.nt(M, 2048, (2368, 512), raw=1)['lds'] and p['ksplit'] == shim.nt(M, 2048, (2368, 512), raw=1)['ksplit']
    assert shim.nt(129, 2048, (2368, 512), **bw)['family'] != NT_BF16W
    assert shim.nt(100, 2048, (2368, 516), **bw)['family'] != NT_BF16W
    assert shim.nt(100, 2048, (2368, 512), f32=1, **bw)['family'] == NT_TILED
    assert shim.nt(100, 2048, (2368, 512), packed=1)['family'] != NT_BF16W          # not without raw slabs
    p = shim.nt(100, 2048, (2368, 512), raw=1, ksplit_out=1)
    short = shim.nt(100, 2048, (2368, 512), ws=p['ws'] - 1, **bw)
    assert (short['family'], short['status']) == (NT_BF16W, WORKSPACE), short
    assert shim.nt(100, 2048, (2368, 512), raw=1, ws=p['ws'] - 1)['status'] == WORKSPACE


def test_short_reduction_kernel_thresholds(shim):
    fam = lambda *a, **k: shim.nt(*a, **k)['family']
    assert fam(1, 16, 2304) == NT_SMALL and fam(1, 16, 2320) != NT_SMALL             # 144 / 145 chunks
    assert shim.nt(1, 16, 2304)['cpw'] == 18
    assert fam(256, 2048, 32) == NT_SMALL and fam(256, 2064, 32) != NT_SMALL         # 2 048 tiles up to 64 chunks
    assert fam(64, 2048, 1028) == NT_SMALL and fam(64, 2064, 1028) != NT_SMALL       # 512 tiles up to 128 chunks
    assert fam(16, 2048, 2176) == NT_SMALL and fam(16, 2064, 2176) != NT_SMALL       # 128 tiles above
    assert fam(64, 2048, 1024) == NT_SMALL and fam(64, 2064, 1024) == NT_SMALL       # (64 chunks: still the wide cap)
    assert fam(1, 16, (64, 64)) == NT_SMALL and fam(1, 16, (64, 64, 64)) != NT_SMALL   # two segments at the most
    assert fam(1, 16, 64, raw=1) != NT_SMALL
    for extra in (dict(addend=1), dict(r1_s=1), dict(epi=EPI_TANHBWD)):
        assert shim.nt(1, 16, 64, **extra)['extras'] == 1
        assert shim.nt(1, 16, 2320, **extra)['status'] == UNSUPPORTED                # the extras live in this kernel only
    assert shim.nt(1, 16, 64)['extras'] == 0


def test_weight_gradient_thresholds(shim):
    fam = lambda *a, **k: shim.tn(*a, **k)['family']
    assert fam(4096, 128, 128) == TN_SPLIT and fam(4095, 128, 128) == TN_STREAM
    assert fam(4096, 128, 128, f32=1) == TN_TILED and fam(4095, 128, 128, f32=1) == TN_STREAM
    assert fam(4096, 128, 132, f32=1) == TN_TILED and fam(4096, 128, 124, f32=1) == TN_STREAM
    assert fam(4096, 128, 256, ldy=128, f32=1) == TN_TILED and fam(4096, 128, 256, ldy=124, f32=1) == TN_STREAM
    assert fam(257, 384, 256, tn_rows=256) == TN_SPLIT and fam(255, 384, 256, tn_rows=256) == TN_STREAM
    assert fam(257, 384, 260, tn_rows=256) == TN_STREAM
    # the many-row form: 1 024 rows, M % 4, 64 x 64, not where the split kernel runs, and the WHOLE layout in the workspace
    assert fam(1024, 64, 64) == TN_MANY_ROW and fam(1020, 64, 64) == TN_STREAM and fam(1026, 64, 64) == TN_STREAM
    assert fam(1024, 64, 60) == TN_STREAM and fam(1024, 64, 64, big=0) == TN_STREAM and fam(1024, 64, 64, f32=1) == TN_STREAM
    assert fam(1024, 128, 128, tn_rows=1024) == TN_SPLIT and fam(1024, 128, 128, tn_rows=1025) == TN_MANY_ROW
    p = shim.tn(1024, 64, 64)
    assert (p['splits'], p['off_xt'], p['off_slabs'], p['ws']) == (8, 65536, 131072, 131072 + 8 * 4096)
    assert fam(1024, 64, 64, ws=p['ws']) == TN_MANY_ROW and fam(1024, 64, 64, ws=p['ws'] - 1) == TN_STREAM
    # every row split degrades to none on a short workspace
    for M, P, Q, sw in ((4096, 128, 128, {}), (4096, 128, 132, dict(f32=1)), (128, 64, 16, {})):
        p = shim.tn(M, P, Q, **sw)
        assert p['splits'] > 1 and p['ws'] == p['splits'] * P * Q
        q = shim.tn(M, P, Q, ws=p['ws'] - 1, **sw)
        assert (q['family'], q['splits'], q['ws']) == (p['family'], 1, 0)
    # the column cut, only if the tail's slabs fit
    p = shim.tn(512, 2048, 4352)
    assert (p['family'], p['q_main'], p['main_columns']) == (TN_COLUMN_CUT, 4096, 4096)
    assert (p['main']['family'], p['main']['splits'], p['tail']['family'], p['tail']['splits']) == (TN_STREAM, 1, TN_STREAM, 8)
    assert shim.tn(512, 2048, 4352, ws=8 * 2048 * 256 - 1)['family'] == TN_STREAM
    assert shim.tn(511, 2048, 4352)['family'] == TN_STREAM and shim.tn(511, 2048, 4352)['main_columns'] == 4352


def test_bias_gradient_and_data_gradient_plans(shim):
    assert shim.colsum(127, 64)['ms'] == 1 and shim.colsum(128, 64)['ms'] == 2
    assert shim.colsum(4096, 64)['ms'] == 32 and shim.colsum(4096, 64, ws=32 * 64 - 1)['ms'] == 1
    assert shim.colsum(4096, 16384 + 1) == dict(ms=1, gx=257, gy=1, fx=65, ws=0)
    p = shim.nn(113, 64, 256)                                # dx [113, 64] over a reduction of 256: 16 chunks, 4 splits
    assert (p['mt'], p['mblocks'], p['ks'], p['ws']) == (7, 2, 4, 4 * 113 * 64)
    assert shim.nn(113, 64, 48)['ks'] == 1                   # (at least four chunks per split)
    q = shim.nn(113, 64, 256, ws=p['ws'] - 1)                # degrade to one split when the workspace is short
    assert (q['mt'], q['ks'], q['ws'], q['gy']) == (7, 1, 0, 1)
    assert [shim.nn(M, 16, 64)['mt'] for M in (16, 17, 32, 33, 64, 65, 112, 113)] == [1, 2, 2, 4, 4, 7, 7, 7]


def test_grouped_weight_gradients(shim):
    M, H, D, F = 2000, 512, 256, 2176
    dgates, xin, h0 = 1, 2, 3                                 # operands by number: the same number, the same buffer
    q_main = shim.tn(M, 4 * H, 2 * F)['main_columns']
    assert q_main == 4096
    jobs = [(M, 4 * H, 2 * F - q_main, 4 * H, 2 * F, dgates, xin + 1000), (M, 4 * H, H, 4 * H, H, dgates, h0),
            (M, D, F, D, F, 4, 5), (M, D, H, D, H, 6, h0), (M, H, 2 * H, H, 2 * H, 7, 8), (M, H, H, H, 2 * H, 9, 8 + 100),
            (M, D, F, D, F, 10, 11), (M, D, H, D, H, 12, 13)]       # the follower's eight decoder gradients
    g = shim.tn_group(jobs, ws=(256 << 20) // 4)
    assert (g['grouped'], g['n'], g['reduce']) == (1, 8, 1)
    assert [j['job'] for j in g['jobs']] == list(range(8))
    assert g['ntr'] == 14                                     # dgates and h0 are shared: transposed once each
    assert g['jobs'][0]['yt'] == g['jobs'][1]['yt'] and g['jobs'][1]['xt'] == g['jobs'][3]['xt']
    offs = [t['off'] for t in g['tr']] + [j['off_slabs'] for j in g['jobs'] if j['ks'] > 1]
    assert offs == sorted(offs) and len(set(offs)) == len(offs) and all(o % 64 == 0 for o in offs) and g['ws'] > offs[-1]
    tiles = sum(-(-j[1] // 128) * -(-j[2] // 128) for j in jobs)
    assert all(j['ks'] == max(1, min(16, 768 // tiles, -(-M // 32) // 4)) for j in g['jobs'])
    # not grouped: a short workspace, one qualifying job, the switch; more than eight: the first eight
    assert shim.tn_group(jobs, ws=g['ws'])['grouped'] == 1 and shim.tn_group(jobs, ws=g['ws'] - 1)['grouped'] == 0
    assert shim.tn_group(jobs[:1], ws=g['ws'])['grouped'] == 0 and shim.tn_group(jobs[:2], ws=g['ws'])['grouped'] == 1
    assert shim.tn_group(jobs, ws=g['ws'], tn_group=0)['grouped'] == 0 and shim.tn_group(jobs, ws=0)['grouped'] == 0
    small = (33, 64, 64, 64, 64, 20, 21)                      # not a many-row product: left to gemm_tn
    g9 = shim.tn_group([small] + jobs + jobs[:1], ws=(256 << 20) // 4)
    assert g9['grouped'] == 1 and [j['job'] for j in g9['jobs']] == list(range(1, 9))
    assert shim.tn_group([small, jobs[1], small], ws=g['ws'])['grouped'] == 0


# ----------------------------------------------------------------------------------------- sweep
SWEEP_M = list(range(1, 601)) + [1024, 2000, 2560, 4096, 4097]
SWEEP_N = (16, 20, 64, 128, 130, 2044, 2048, 2176)
SWEEP_K = (4, 32, 300, 1024, 1028, 2176, 2320, 2368, 4352)
SWEEP_ASKS = (dict(), dict(f32=1), dict(raw=1, ksplit_out=1), dict(raw=1, ksplit_out=1, packed=1), dict(raw=1, f32=1))


def check_nt_plan(shim, p, offered, what):
    if p['status'] != OK:
        assert p['status'] in (UNSUPPORTED, WORKSPACE), (what, p)
        return
    if p['family'] == NT_SMALL:
        assert (p['mt'], p['cpw']) in shim.small_insts, (what, p)
    elif p['family'] != NT_BIG:
        assert 1 <= p['mt'] <= shim.nt_mt_max, (what, p)
    assert p['family'] in range(6) and min(p['gx'], p['gy'], p['gz']) >= 1 and p['block'] in (256, 512), (what, p)
    assert p['ws'] <= offered and p['ksplit'] >= 1 and p['lds'] <= 160 * 1024, (what, p)
    assert not (p['reduce'] and not p['slabs']), (what, p)


@pytest.mark.parametrize('ask', range(len(SWEEP_ASKS)), ids=['fwd', 'fwd-f32', 'slabs', 'slabs-bf16w', 'slabs-f32'])
def test_sweep_names_only_what_exists(shim, ask):
    kw = SWEEP_ASKS[ask]
    for M in SWEEP_M:
        for N in SWEEP_N:
            for K in SWEEP_K:
                check_nt_plan(shim, shim.nt(M, N, K, ws=WS, **kw), WS, (M, N, K, kw))
                check_nt_plan(shim, shim.nt(M, N, K, ws=M * N, **kw), M * N, (M, N, K, kw))


def test_sweep_of_the_data_gradient_and_its_sizing(shim):
    for M in SWEEP_M:
        for N in SWEEP_N:
            for K in SWEEP_K:
                p, short = shim.nn(M, N, K, ws=AMPLE), shim.nn(M, N, K, ws=M * N)
                assert p['sizing'] == p['ws'], (M, N, K, p)                   # gemm_nn_ws_floats is the plan's figure
                for q, offered in ((p, AMPLE), (short, M * N)):
                    assert q['mt'] in shim.nn_insts and min(q['gx'], q['gy'], q['gz']) >= 1, (M, N, K, q)
                    assert q['ws'] <= offered and q['ks'] >= 1 and q['gy'] == q['ks'], (M, N, K, q)
