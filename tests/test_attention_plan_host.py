"""The attention dispatch asked on the host: csrc/sf_attention_plan.h holds the shape rules of the row-set kernels, what each
paired launch accepts of its small products and the ladders that pick a template value -- pure C++ that includes no HIP
header -- and the launchers of csrc/sf_attention.hip and the chains of csrc/sf_api_follower.hip only ask it.
tests/attention_plan_shim.cpp wraps it; it is compiled here with g++ and loaded with ctypes.  No GPU, no HIP, nothing of the
library itself is loaded.

Expectations are the rules written down: tests/attention_cases.py (the tables the GPU module runs) and the literal figures
below.  None is read from the header under test."""
import ctypes as C
import os
import subprocess

import pytest

from tests import attention_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED = 0, 2
MTS, CPWS = range(1, 9), (1, 2, 4, 8, 16)
SMALL_SMALL, TEXTFOLD, APRO_SMALL, SMALL_TEXT, VISBWD_SMALL, PROJ_TEXTFOLD, VIS_SMALL = range(7)
PANORAMA = dict(IMG=2048, LOC=128)                    # the follower's rows: F = 2176


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp('attention_plan') / 'attention_plan_shim.so'
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-shared', '-fPIC',
                    '-I' + os.path.join(ROOT, 'speaker_follower_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'attention_plan_shim.cpp'), '-o', str(so)], check=True)
    return Shim(C.CDLL(str(so)))


def rows(n, F=None, IMG=0, LOC=0, half=0):
    """A row source as the rules see it: dense rows of F floats, or the index form IMG + LOC."""
    return (C.c_int * 5)(n, F if F is not None else IMG, 0 if F is not None else LOC, int(F is not None), half)


class Shim:
    def __init__(self, lib):
        self.lib = lib
        lib.shim_visual_attn_split_floats.restype = lib.shim_text_fold_part_floats.restype = C.c_longlong
        t = (C.c_int * 64)()
        n = lib.shim_tables(t)
        names = ('VIS_CPL VIS_RPW VIS_NW VSP_G VSP_RPG VIS_SPLIT_MAX_B TXT_CPL TXT_NW SC_CPL SC_NW CG_ROWS TXT_MAX_L '
                 'TXF_G TXF_MAX_L TXF_MAX_B TXF_G2_MAX_L PRJ_CPL PPB_G SPLIT_MAX_G SMALL_WAVES').split()
        assert n == len(names)
        self.const = dict(zip(names, t[:n]))

    def __getattr__(self, name):
        f = getattr(self.lib, 'shim_' + name)
        return lambda *a: f(*a)

    def accepted(self, which, phase=0, a=None):
        """The (mt, cpw) a launcher accepts over the sweep -- of its second product when the first is `a`."""
        if a is None:
            return {(m, c) for m in MTS for c in CPWS if self.lib.shim_accepts(which, m, c, 0, 0, phase)}
        return {(m, c) for m in MTS for c in CPWS if self.lib.shim_accepts(which, a[0], a[1], m, c, phase)}

    def groups(self, B, L, partials=1, na=32, slots=512, force=0):
        grid = C.c_int(-1)
        return self.lib.shim_proj_text_groups_plan(B, L, partials, na, slots, force, C.byref(grid)), grid.value


# ------------------------------------------------------------------------------ the tables of attention_cases
def test_constants_are_the_ones_the_cases_mirror(shim):
    c = shim.const
    assert (c['VIS_CPL'], c['VIS_RPW'], c['VIS_NW']) == (A.VIS_CPL, A.VIS_RPW, A.VIS_NW)
    assert (c['VSP_G'], c['VSP_RPG'], c['VIS_SPLIT_MAX_B']) == (A.VSP_G, A.VSP_RPG, A.VIS_SPLIT_MAX_B)
    assert (c['TXT_CPL'], c['TXT_NW'], c['TXT_MAX_L']) == (A.TXT_CPL, A.TXT_NW, A.L_MAX)
    assert (c['SC_CPL'], c['SC_NW'], c['CG_ROWS']) == (A.SC_CPL, A.SC_NW, A.CG_ROWS)
    assert (c['TXF_MAX_L'], c['TXF_MAX_B'], c['TXF_G2_MAX_L']) == (160, 512, 80)
    assert (c['TXF_G'], c['PRJ_CPL'], c['PPB_G'], c['SPLIT_MAX_G'], c['SMALL_WAVES']) == (4, 2, 3, 3, 8)


def visual_kernel(shim, src, V, B, workspace=True):
    assert shim.pano_rows_fit(src) == 1
    return A.VIS_SPLIT if workspace and shim.in_split_range(V, B) else A.VIS_FWD


def test_visual_cases_reach_the_kernels_they_name(shim):
    for c in A.VISUAL:
        assert visual_kernel(shim, rows(c.V, c.F), c.V, c.B) == c.kernel == A.visual_fwd_kernel(c.V, c.B), c
        assert visual_kernel(shim, rows(c.V, c.F), c.V, c.B, workspace=False) == A.visual_fwd_kernel(c.V, c.B, False), c
        assert bool(shim.split_rows_fit(rows(c.V, c.F), c.B)) == A.visual_f64_supported(c.V, c.B, c.F), c
    for c in A.VISUAL_INDEX:
        src = rows(c.V, IMG=c.IMG, LOC=c.LOC)
        assert visual_kernel(shim, src, c.V, c.B) == c.kernel == A.visual_fwd_kernel(c.V, c.B), c
    for c in A.VISUAL_BWD:                                   # (the backward is never split: the rows only have to fit)
        assert shim.pano_rows_fit(rows(c.V, c.F)) == 1, c
    for c in A.VISUAL_F64:
        assert shim.split_rows_fit(rows(c.V, c.F), c.B) == 1 and A.visual_f64_supported(c.V, c.B, c.F), c


def test_text_score_and_context_gradient_cases(shim):
    for c in A.TEXT:
        assert shim.text_rows_fit(c.L, A.L_MAX, c.H, 0) == 1, c
        assert A.TXT % shim.text_rpw(c.L) == c.kernel == A.text_kernel(c.L), c
    for L in range(1, A.L_MAX + 40):
        assert (A.TXT % shim.text_rpw(L) if shim.text_rpw(L) else None) == A.text_kernel(L), L
    for c in A.SCORE:
        assert shim.cand_rows_fit(rows(c.A, c.F)) == 1, c
    for c in A.SCORE_INDEX:
        assert shim.cand_rows_fit(rows(c.A, IMG=c.IMG, LOC=c.LOC)) == 1, c
    for c in A.CTX_GRAD:
        assert bool(shim.ctx_grad_supported(c.S, c.L, 512)) == c.runs == A.ctx_grad_supported(c.S, c.L, 512), c
    for H in (0, 4, 6, 12, 256, 512, 516, 1024, 4096, 4100):
        for L in (1, 20, 80, 81, 160, 161, 2560, 2561):
            for S in (1, 102, 103, 8192, 8193):
                assert bool(shim.ctx_grad_supported(S, L, H)) == A.ctx_grad_supported(S, L, H), (S, L, H)


def test_refusals_get_the_status_they_name(shim):
    """A launcher's gate is `every named rule holds`, SF_ERR_UNSUPPORTED otherwise (csrc/sf_attention.hip: visual_attn,
    text_attn_fwd, score_fwd); every leading dimension not named by the case is the row width."""
    for r in A.REFUSALS:
        d = r.dims
        if r.entry == 'visual':
            ok = shim.pano_rows_fit(rows(d['V'], d['F'])) and shim.aligned4(d['F'], d.get('ldo', d['F']), 0)
        elif r.entry == 'text':
            ok = shim.text_rows_fit(d['L'], A.L_MAX, d['H'], d['H'] | 2 * d['H'])
        else:
            ok = shim.cand_rows_fit(rows(d['A'], d['F']))
        assert (OK if ok else UNSUPPORTED) == r.status, r
    assert len(A.REFUSALS) == 9


# ------------------------------------------------------------------------------------ thresholds
def test_split_range_thresholds(shim):
    fits = lambda V, B=100: (shim.in_split_range(V, B), shim.split_rows_fit(rows(V, **PANORAMA), B))
    assert fits(18) == (0, 0) and fits(19) == (1, 1) and fits(36) == (1, 1) and fits(37) == (0, 0)
    assert fits(36, 256) == (1, 1) and fits(36, 257) == (0, 0)
    assert shim.pano_rows_fit(rows(36, **PANORAMA)) == 1 and shim.pano_rows_fit(rows(37, **PANORAMA)) == 0
    assert shim.pano_rows_fit(rows(0, **PANORAMA)) == 1                              # (no lower limit outside the split)


def test_row_width_thresholds(shim):
    for fit, n in ((shim.pano_rows_fit, 36), (shim.cand_rows_fit, 16)):
        assert fit(rows(n, 2304)) == 1 and fit(rows(n, 2308)) == 0
        assert fit(rows(n, 2302)) == 0 and fit(rows(n, 4)) == 1                        # F % 4
        assert fit(rows(n, IMG=2176, LOC=128)) == 1 and fit(rows(n, IMG=2176, LOC=132)) == 0
        assert fit(rows(n, IMG=2050, LOC=126)) == 0 and fit(rows(n, 2176)) == 1        # index form: each part % 4
    # index-form LOC: a multiple of 4 but not of 16 passes the panorama rule and fails the candidate rule
    assert shim.pano_rows_fit(rows(16, IMG=2048, LOC=132)) == 1 and shim.cand_rows_fit(rows(16, IMG=2048, LOC=132)) == 0
    assert shim.cand_rows_fit(rows(16, IMG=2048, LOC=144)) == 1 and shim.cand_rows_fit(rows(16, 2048 + 132)) == 1
    assert shim.cand_rows_fit(rows(16, **PANORAMA)) == 1 and shim.cand_rows_fit(rows(17, **PANORAMA)) == 0   # A
    assert shim.cand_rows_fit(rows(1, **PANORAMA)) == 1 and shim.cand_rows_fit(rows(0, **PANORAMA)) == 0


def test_text_thresholds(shim):
    text = lambda L, Lmax, H=512, lds=0: shim.text_rows_fit(L, Lmax, H, lds)
    assert text(1, 128) == 1 and text(0, 128) == 0
    assert text(128, 128) == 1 and text(129, 128) == 0
    assert text(160, 160) == 1 and text(161, 160) == 0
    assert text(40, 128, H=512) == 1 and text(40, 128, H=516) == 0 and text(40, 128, H=510) == 0          # H
    assert text(40, 128, lds=1024 | 512) == 1 and text(40, 128, lds=1024 | 514) == 0
    # the folded text stage: L 160 / 161, B 512 / 513, z at least H wide
    fold = lambda B, L, H=512, ldvec=1024, ldz=528: shim.text_fold_fits(B, L, H, ldvec, ldz)
    assert fold(512, 160) == 1 and fold(513, 160) == 0 and fold(512, 161) == 0 and fold(512, 0) == 0
    assert fold(100, 80, ldz=512) == 1 and fold(100, 80, ldz=508) == 0 and fold(100, 80, ldz=530) == 0
    assert fold(100, 80, ldvec=1026) == 0 and fold(100, 80, H=516, ldz=532) == 0


def test_ladders(shim):
    ladder = lambda f, *a: [f(L, *a) for L in range(1, 170)]
    want = lambda steps: [next((v for top, v in steps if L <= top), 0) for L in range(1, 170)]
    assert ladder(shim.text_rpw) == want(((16, 1), (80, 5), (128, 8)))               # L, text: 16/17, 80/81, 128/129
    assert ladder(shim.fold_rpw, 4) == want(((32, 1), (64, 2), (96, 3), (10 ** 6, 5)))   # L, fold: 32/33, 64/65, 96/97 (160: the gate)
    assert ladder(shim.fold_rpw, 2) == want(((16, 1), (32, 2), (48, 3), (10 ** 6, 5)))   # two text groups: 80 = 2 x 8 x 5 is the gate
    assert [shim.text_rung(L, 4) for L in (32, 33, 64, 65, 96, 97, 160)] == [0, 1, 1, 2, 2, 3, 3]
    assert shim.text_rpw(128) and not shim.text_rpw(129)                             # a ladder ends where its gate does
    assert shim.const['TXF_MAX_L'] == 4 * 8 * 5 and shim.const['TXF_G2_MAX_L'] == 2 * 8 * 5


def test_scratch_sizes(shim):
    assert shim.visual_attn_split_floats(100, 2176) == 100 * 3 * (2176 + 64)          # three records: the projected partials
    assert shim.text_fold_part_floats(100, 512) == 100 * 4 * (512 + 64)
    assert shim.visual_attn_split_floats(1 << 20, 2304) == (1 << 20) * 3 * 2368       # (past 2^31: size_t)


def test_projected_chain_rule(shim):
    us, xn = rows(8, **PANORAMA), rows(36, **PANORAMA)
    chain = lambda us=us, xn=xn, B=100, H=512, L=80, tH=512, tld=528: shim.proj_chain_supported(us, xn, B, H, L, tH, tld)
    assert chain() == 1 and chain(xn=None) == 1
    assert chain(B=256) == 1 and chain(B=257) == 0 and chain(B=257, xn=None) == 0 and chain(B=0) == 0
    assert chain(L=160) == 1 and chain(L=161) == 0 and chain(L=0) == 0
    assert chain(H=516, tH=516, tld=532) == 0 and chain(H=0, tH=0, tld=16) == 0 and chain(tH=256) == 0
    assert chain(tld=512) == 0 and chain(tld=513) == 0 and chain(tld=516) == 1
    assert chain(us=rows(16, **PANORAMA)) == 1 and chain(us=rows(17, **PANORAMA)) == 0
    # the index form is required: dense or binary16 candidates, or a panorama of either kind, decline
    assert chain(us=rows(8, 2176)) == 0 and chain(us=rows(8, half=1, **PANORAMA)) == 0
    assert chain(xn=rows(36, 2176)) == 0 and chain(xn=rows(36, half=1, **PANORAMA)) == 0
    assert chain(xn=rows(18, **PANORAMA)) == 0 and chain(xn=rows(19, **PANORAMA)) == 1 and chain(xn=rows(37, **PANORAMA)) == 0
    assert chain(xn=rows(36, IMG=2048, LOC=144)) == 0                                 # candidates and panorama: one layout
    assert chain(us=rows(8, IMG=2048, LOC=132), xn=rows(36, IMG=2048, LOC=132)) == 0
    # launch (1) carries the partials where image and location chunks fit a lane's nine slots side by side
    assert shim.proj_partials_supported(2048, 128) == 1 and shim.proj_partials_supported(0, 128) == 0
    assert shim.proj_partials_supported(2048, 256) == 1 and shim.proj_partials_supported(2048, 260) == 0


# -------------------------------------------------------------------------- accepted (mt, cpw) sets
ONE_TWO_FOUR = (1, 2, 4)


def test_accepted_small_products(shim):
    assert shim.accepted(SMALL_SMALL, a=(1, 4)) == {(m, 4) for m in ONE_TWO_FOUR}
    # the folded text stage: t_v' beside y is (1, 4) and nothing else -- (2, 4) and (4, 4), which only the retired
    # three-launch chain planned (its q' product over F columns), are refused
    assert shim.accepted(TEXTFOLD, a=(1, 4)) == {(1, 4)}
    assert not shim.lib.shim_accepts(TEXTFOLD, 1, 4, 2, 4, 0) and not shim.lib.shim_accepts(TEXTFOLD, 1, 4, 4, 4, 0)
    assert shim.accepted(APRO_SMALL, a=(1, 4)) == {(m, 2) for m in ONE_TWO_FOUR}
    for which in (SMALL_SMALL, TEXTFOLD, APRO_SMALL):                                 # a = (1, 4) and nothing else
        for a in ((m, c) for m in MTS for c in CPWS if (m, c) != (1, 4)):
            assert shim.accepted(which, a=a) == set(), (which, a)
    assert shim.accepted(SMALL_TEXT) == {(4, 2)}
    assert shim.accepted(VISBWD_SMALL) == {(1, 16)}
    assert shim.accepted(PROJ_TEXTFOLD) == {(1, 4)}
    for phase in (0, 1):
        assert shim.accepted(VIS_SMALL, phase) == {(m, 2) for m in ONE_TWO_FOUR} | {(1, 8)}
    assert shim.accepted(VIS_SMALL, 2) == {(1, 8), (1, 4)}
    assert shim.accepted(VIS_SMALL, 3) == set() and shim.accepted(VIS_SMALL, -1) == set()
    t = (C.c_int * 64)()
    n = shim.vis_small_insts(t)
    insts = {(t[3 * i], t[3 * i + 1], t[3 * i + 2]) for i in range(n)}
    assert n == len(insts) == 10 and insts == {(m, c, p) for p in (0, 1, 2) for m, c in shim.accepted(VIS_SMALL, p)}


# ------------------------------------------------------------------------ text groups of launch (1)
def test_text_groups_of_the_projected_launch(shim):
    g = shim.groups
    assert g(68, 80) == (4, 508) and g(69, 80) == (2, 3 * 69 + 2 * 69 + 32)           # the first batch over 512 slots
    assert g(100, 80) == (2, 532) and g(100, 1) == (2, 532) and g(16, 80) == (4, 7 * 16 + 32)
    assert g(100, 81) == (4, 732) and g(100, 160) == (4, 732)                         # L, two text groups: 80 / 81
    assert g(100, 80, partials=0) == (4, 432) and g(256, 20, partials=0) == (4, 4 * 256 + 32)
    assert g(1, 80) == (4, 7 + 32) and g(256, 80) == (2, 5 * 256 + 32)
    assert g(100, 80, slots=0) == (4, 732)                                           # unknown slots: four
    groups = [g(B, 40)[0] for B in range(1, 257)]
    assert groups.index(2) + 1 == 69 and set(groups[:68]) == {4} and set(groups[68:]) == {2}
    # forced: 2 only where two is legal (partials in the launch, L <= 80), 4 always, anything else the rule
    assert g(16, 80, force=2) == (2, 5 * 16 + 32) and g(16, 81, force=2)[0] == 4 and g(16, 80, partials=0, force=2)[0] == 4
    assert g(100, 80, force=4) == (4, 732) and g(100, 80, force=3) == (2, 532) and g(16, 80, force=3)[0] == 4
    assert shim.lib.shim_proj_text_groups_plan(100, 80, 1, 32, 512, 0, None) == 2     # (the grid is optional)
