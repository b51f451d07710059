"""HBM-resident image-feature store and index-form observations.

Replaces the reference's per-step host work -- dict lookup of a 36x2048 block per
sample (env.py:380-383), concatenation with the location embedding (env.py:773),
construction of the candidate-action embeddings (env.py:60-75), np.stack and the
H2D copy (env.py:330-332, follower.py:291-320) -- by ONE [n_viewpoints,36,2048]
fp32 tensor that lives in HBM (3.1 GB for the full R2R set; 288 GB available) plus a
36x36x128 location table; per step only a few int32 indices per sample travel.
"""
import base64
import csv
import ctypes as C
import json
import sys
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import call
from .runtime import ptr, stream

NUM_VIEWS = 36          # env.py:285
MEAN_POOLED_DIM = 2048  # env.py:286
LOC_DIM = 128           # env.py:62, 87
ANGLE_INC = np.pi / 6.0  # env.py:57


def build_loc_table(n_views=NUM_VIEWS, loc=LOC_DIM):
    """[n_views (agent view index), n_views (absolute view), loc]: sin/cos of each view's
    heading / elevation relative to the agent's view (env.py:78-101, 12 headings x 3
    elevations), each repeated loc/4 times."""
    g = loc // 4
    tab = np.zeros((n_views, n_views, loc), np.float32)
    for view in range(n_views):
        for abs_view in range(n_views):
            rel = (abs_view - view) % 12 + (abs_view // 12) * 12
            h = (rel % 12) * ANGLE_INC
            e = (rel // 12 - 1) * ANGLE_INC
            tab[view, abs_view, 0:g] = np.sin(h)
            tab[view, abs_view, g:2 * g] = np.cos(h)
            tab[view, abs_view, 2 * g:3 * g] = np.sin(e)
            tab[view, abs_view, 3 * g:] = np.cos(e)
    return tab


def cand_sincos(rel_heading, rel_elevation):
    """[..., 4] fp32 = sin h, cos h, sin e, cos e, evaluated in float64 like the
    reference does on the simulator's python floats (env.py:69-74)."""
    h = np.asarray(rel_heading, np.float64)
    e = np.asarray(rel_elevation, np.float64)
    return np.stack((np.sin(h), np.cos(h), np.sin(e), np.cos(e)), axis=-1).astype(np.float32)


def gate_loc_groups(w_loc):
    """[4, N] float64 from the location columns w_loc [N, loc] of a weight applied to candidate rows: row k is the sum of
    block k (loc/4 contiguous columns) -- the k-th of `cand_sincos`'s four values fills exactly that block of a candidate
    row, so the location part contributes sum_k sincos_k * row k.  What the library's `gl` table holds (sf_gate_rows_build)."""
    w = np.asarray(w_loc, np.float64)
    g = w.shape[1] // 4
    return np.stack([w[:, k * g:(k + 1) * g].sum(axis=1) for k in range(4)])


DTYPES = {'fp32': torch.float32, 'fp16': torch.float16}
FILE_DTYPES = {'fp32': 'float32', 'fp16': 'float16'}     # the "dtype" key of '<bin>.json' (absent: float32)
CHECK_ROWS = 256        # viewpoint rows rounded / checked at a time (never a second copy of the whole table)


def _dtype_name(dtype):
    if dtype not in DTYPES:
        raise ValueError("dtype must be 'fp32' or 'fp16' (got %r)" % (dtype,))
    return dtype


def round_to_fp16(rows, row0=0):
    """fp32 [r, V, IMG] tensor -> torch.float16 by torch's own conversion (round to nearest even).  The kernels blend
    table rows with x * 0 and rely on finite features, so a NaN in the input or a magnitude that rounds to inf is a
    ValueError naming the first offending row (`row0` + its index in `rows`)."""
    half = rows.to(torch.float16)
    bad = ~torch.isfinite(half.reshape(half.shape[0], -1)).all(dim=1)
    if bool(bad.any()):
        r = int(torch.nonzero(bad)[0, 0])
        raise ValueError('feature table row %d does not fit fp16 storage: it holds a NaN, an infinity or a magnitude '
                         'that rounds to infinity (fp16 max is 65504)' % (row0 + r))
    return half


def tsv_to_bin(tsv_path, bin_path, dtype='fp32'):
    """One-shot converter (N4): the reference's ResNet TSV -> flat little-endian fp32 file
    [n][36][2048] + '<bin>.json' {ids, shape}.  Streams row by row (the full table is 3.1 GB).
    dtype='fp16' writes binary16 rows (rounded like FeatureStore(dtype='fp16') rounds) and records
    "dtype": "float16" in the json; a json without the key describes an fp32 file."""
    half = _dtype_name(dtype) == 'fp16'
    csv.field_size_limit(sys.maxsize)
    names = ['scanId', 'viewpointId', 'image_w', 'image_h', 'vfov', 'features']
    ids = []
    with open(tsv_path, 'rt') as f, open(bin_path, 'wb') as out:
        for item in csv.DictReader(f, delimiter='\t', fieldnames=names):
            buf = base64.b64decode(item['features'])
            if len(buf) != NUM_VIEWS * MEAN_POOLED_DIM * 4:
                raise ValueError('row %s_%s: %d feature bytes' % (item['scanId'], item['viewpointId'], len(buf)))
            if half:
                row = torch.from_numpy(np.frombuffer(buf, np.float32).reshape(1, NUM_VIEWS, MEAN_POOLED_DIM).copy())
                buf = round_to_fp16(row, len(ids)).numpy().tobytes()
            out.write(buf)
            ids.append(item['scanId'] + '_' + item['viewpointId'])
    meta = {'ids': ids, 'shape': [len(ids), NUM_VIEWS, MEAN_POOLED_DIM]}
    if half:
        meta['dtype'] = FILE_DTYPES['fp16']
    with open(bin_path + '.json', 'w') as f:
        json.dump(meta, f)
    return len(ids)


def _forget_projected(addr, pv):
    """Drops the library's projected-table entry of the table at `addr` -- when `pv` is given, only if it still is the
    entry whose pv table lives there (a collected decoder must not unregister the tables of another one)."""
    if pv is not None:
        cur = _lib.Projected()
        if not _lib.lib.sf_projected_registered(C.c_void_p(addr), C.byref(cur)) or cur.pv != pv:
            return
    _lib.lib.sf_projected_register(C.c_void_p(addr), None)


def _forget_gate_rows(addr, gu):
    """The same for the gate-space rows of the table at `addr` (`gu`: only if its gu table still lives there)."""
    if gu is not None:
        cur = _lib.GateRows()
        if not _lib.lib.sf_gate_rows_registered(C.c_void_p(addr), C.byref(cur)) or cur.gu != gu:
            return
    _lib.lib.sf_gate_rows_register(C.c_void_p(addr), None)
    _lib.lib.sf_gate_rows_attended_register(C.c_void_p(addr), None)      # (the attended half lives and dies with them)


class FeatureStore:
    """The feature table in HBM + viewpoint-id index.

    dtype='fp16' keeps the table as torch.float16 (half the HBM bytes and half of what every table kernel reads): it
    is rounded ONCE, with torch's `.to(torch.float16)`, and the kernels widen each value exactly as they load it, so
    the store behaves bit for bit like an fp32 store built from `table.half().float()`.  `table` stays the device
    tensor in its storage dtype (`rows_f32` widens rows); the location table, the dense materialisations and every
    output are fp32.  The library knows an fp16 table by its address (sf_feature_table_f16): the store registers it
    here and forgets it when it is collected, so a store must outlive every captured graph that ran with it -- as it
    must for its memory anyway."""

    def __init__(self, table, ids=None, device='cuda', loc=LOC_DIM, dtype='fp32'):
        self.dtype = _dtype_name(dtype)
        if isinstance(table, np.ndarray):
            if table.dtype != np.float16:
                table = np.ascontiguousarray(table, np.float32)
            table = torch.from_numpy(np.ascontiguousarray(table))
        if table.dim() != 3:
            raise ValueError('feature table must be [n, V, IMG] (got %s)' % (tuple(table.shape),))
        if self.dtype == 'fp16' and table.dtype != torch.float16:
            # rounded and checked chunk by chunk into the one preallocated fp16 tensor
            out = torch.empty(table.shape, dtype=torch.float16, device=device)
            for r0 in range(0, table.shape[0], CHECK_ROWS):
                out[r0:r0 + CHECK_ROWS].copy_(round_to_fp16(table[r0:r0 + CHECK_ROWS].to(torch.float32), r0))
            self.table = out
        else:
            self.table = table.to(device=device, dtype=DTYPES[self.dtype]).contiguous()
            if self.dtype == 'fp16':            # already binary16 (from_bin): nothing to round, finiteness still holds
                for r0 in range(0, self.table.shape[0], CHECK_ROWS):
                    round_to_fp16(self.table[r0:r0 + CHECK_ROWS], r0)
        self.n, self.V, self.IMG = self.table.shape
        if self.dtype == 'fp16' and self.IMG % 4:
            raise ValueError('fp16 storage needs IMG %% 4 == 0 (got %d)' % self.IMG)
        # The library tells the storage by the table's ADDRESS.  An fp32 store clears its address too: the caching
        # allocator can hand the address of a collected fp16 table to an fp32 one.
        if self.table.numel():
            addr = self.table.data_ptr()
            call('sf_feature_table_f16', C.c_void_p(addr), 1 if self.dtype == 'fp16' else 0)
            if self.dtype == 'fp16':
                weakref.finalize(self, _lib.lib.sf_feature_table_f16, C.c_void_p(addr), 0)
            # ... and a projected-table entry of a collected store that lived at this address (`projected` below)
            call('sf_projected_register', C.c_void_p(addr), None)
            call('sf_gate_rows_register', C.c_void_p(addr), None)
            call('sf_gate_rows_attended_register', C.c_void_p(addr), None)
        self._projected = weakref.WeakKeyDictionary()       # decoder module -> its projected tables (see `projected`)
        self._gate_rows = weakref.WeakKeyDictionary()       # decoder module -> its gate-space rows (see `gate_rows`)
        self.LOC = loc
        self.F = self.IMG + loc
        self.device = self.table.device
        self.loc_table = torch.from_numpy(build_loc_table(self.V, loc)).to(self.device)
        self.index = {k: i for i, k in enumerate(ids)} if ids is not None else None

    @classmethod
    def from_tsv(cls, path, device='cuda', dtype='fp32'):
        """Reads the reference's ResNet-152 TSV (scanId, viewpointId, image_w, image_h, vfov,
        base64 fp32 36x2048; env.py:359-370, scripts/precompute_img_features.py:31)."""
        csv.field_size_limit(sys.maxsize)
        names = ['scanId', 'viewpointId', 'image_w', 'image_h', 'vfov', 'features']
        ids, rows = [], []
        with open(path, 'rt') as f:
            for item in csv.DictReader(f, delimiter='\t', fieldnames=names):
                ids.append(item['scanId'] + '_' + item['viewpointId'])       # env.py:377-378
                buf = base64.b64decode(item['features'])
                rows.append(np.frombuffer(buf, np.float32).reshape(NUM_VIEWS, MEAN_POOLED_DIM))
        return cls(np.stack(rows), ids, device, dtype=dtype)

    @classmethod
    def from_bin(cls, path, device='cuda', chunk_rows=512, dtype=None):
        """Flat table written by `tsv_to_bin` (path + '.json' holds the ids and shape): the file is
        memory-mapped and uploaded in chunks straight into ONE preallocated HBM tensor, so start-up
        costs a sequential read instead of minutes of TSV / base64 parsing.  dtype=None keeps the
        file's storage (the json's "dtype"; absent: fp32); naming the other one converts chunk by
        chunk during the upload (fp32 -> fp16 rounds and checks like the constructor does)."""
        with open(path + '.json') as f:
            meta = json.load(f)
        n, V, IMG = meta['shape']
        stored = meta.get('dtype', FILE_DTYPES['fp32'])
        if stored not in FILE_DTYPES.values():
            raise ValueError('%s.json: unknown dtype %r' % (path, stored))
        file16 = stored == FILE_DTYPES['fp16']
        dtype = _dtype_name(('fp16' if file16 else 'fp32') if dtype is None else dtype)
        mm = np.memmap(path, dtype=np.float16 if file16 else np.float32, mode='r', shape=(n, V, IMG))
        table = torch.empty(n, V, IMG, dtype=DTYPES[dtype], device=device)
        for r0 in range(0, n, chunk_rows):
            r1 = min(n, r0 + chunk_rows)
            rows = torch.from_numpy(np.array(mm[r0:r1]))
            if dtype == 'fp16':
                rows = round_to_fp16(rows, r0)       # (a binary16 file: only the finiteness check)
            table[r0:r1].copy_(rows)
        return cls(table, meta['ids'], device, dtype=dtype)

    def row(self, scan_id, viewpoint_id):
        return self.index[scan_id + '_' + viewpoint_id]

    def rows_f32(self, idx):
        """table[idx] widened to fp32 (exact), on the table's device."""
        return self.table[idx].to(torch.float32)

    # ---- projected tables (include/sf_hip.h: sf_projected_build) ---------------------------------
    def projected(self, decoder, build=True):
        """The projected feature tables of (this store, `decoder`): every table row carried through the decoder's folded
        query / scoring matrices ONCE, so that an inference decode step needs two dependent launches behind the LSTM cell
        instead of four (include/sf_hip.h).  A derived copy of the weights like `runtime.transposed` and
        `model.decoder_fold`: cached here per decoder, rebuilt IN PLACE (same addresses: a captured hipGraph keeps pointing
        at them) when the version counter of a weight they depend on changes, dropped when the store or the decoder is
        collected.  Costs 2 * n * V * (H + 4) * 4 bytes (1.57 GB for the full R2R table) and about 13 ms on MI355X, which a
        replayed rollout repays and a single one does not: `build=False` returns the tables only if they exist already
        (refreshed), else None.  None for an fp16 store.  Also tells the library that THIS decoder's tables are the ones
        of the table's address (it holds one entry per address)."""
        from .model import decoder_fold, decoder_params          # (model imports this module)
        from .runtime import weight_key, ws_args
        if self.dtype != 'fp32' or not self.table.numel() or self.IMG % 4 or self.LOC % 16:
            return None
        hit = self._projected.get(decoder)
        if hit is None and not build:
            return None
        params = decoder_params(decoder)
        key = weight_key(*(params[i] for i in (4, 5, 6, 10, 11, 12, 13, 14, 15))) + \
            (self.table.data_ptr(), self.table._version, self.loc_table.data_ptr())
        if hit is None or hit['key'] != key:
            H = decoder.hidden_size
            if H % 4 or decoder.feature_size != self.F:
                return None
            ld, rows = int(_lib.lib.sf_projected_ld(H)), self.n * self.V
            new = lambda r: torch.empty(r, ld, device=self.device, dtype=torch.float32)  # noqa: E731
            bufs = hit['bufs'] if hit is not None and hit['bufs'][0].shape == (rows, ld) else \
                (new(rows), new(rows), new(self.V * self.V), new(5))
            fold = decoder_fold(decoder)                           # (itself rebuilt in place per weight version)
            rc = _lib.lib.sf_projected_build(C.byref(fold), ptr(self.table), rows, ptr(self.loc_table), self.V, self.IMG,
                                             self.LOC, H, *(ptr(b) for b in bufs), *ws_args(self.device))
            if rc == _lib.SF_ERR_UNSUPPORTED and hit is None:      # (a shape the products do not take: no tables, no error)
                return None
            _lib.check(rc, 'sf_projected_build')
            struct = _lib.Projected(*(b.data_ptr() for b in bufs), self.loc_table.data_ptr(), params[4].data_ptr(),
                                    params[10].data_ptr(), H, ld, self.V, self.IMG, self.LOC, 0)
            first = hit is None
            hit = dict(key=key, bufs=bufs, struct=struct, builds=(0 if first else hit['builds']) + 1)
            self._projected[decoder] = hit
            if first:
                addr = self.table.data_ptr()
                weakref.finalize(decoder, _forget_projected, addr, bufs[0].data_ptr())
                weakref.finalize(self, _forget_projected, addr, None)
        call('sf_projected_register', C.c_void_p(self.table.data_ptr()), C.byref(hit['struct']))
        return hit

    # ---- gate-space rows (include/sf_hip.h: sf_gate_rows_build) ----------------------------------
    def gate_rows(self, decoder, build=True, attended=True):
        """The gate-space rows of (this store, `decoder`): every table row carried through the action half of the decoder
        LSTM's input weights ONCE (gu [n * V, 4H], gl [4, 4H]), so that a step of the projected chain takes its gate product
        over K = F + H instead of 2 F + H (include/sf_hip.h).  Kept beside the projected tables with the same policy:
        cached per decoder, rebuilt IN PLACE when `weight_ih`'s version counter or the table changes, dropped with the
        store or the decoder, `build=False` returns them only if they exist (refreshed), else None; None for an fp16
        store.  Costs n * V * 4H * 4 bytes (3.1 GB for the full R2R table at H = 512).  The callers ask for them only
        where the projected tables are in use (FollowerEngine).

        `attended` (default on) keeps, in the SAME entry and under the same rules, the table of the other half of the
        input: gf [n * V, 4H], every row through the image columns of the attended feature (sf_gate_rows_attended_build),
        which leaves the product K = LOC + H.  Another n * V * 4H * 4 bytes.  hit['attended'] is dict(buf, struct), or
        None where it was not asked for or launch (1)'s partials do not take rows of 4H + LOC floats; one `builds` count
        covers both tables.  The table is ADDED only where `build` is true (the first build, or a caller that builds and
        asks for it behind an entry made without it); a refresh keeps what the entry holds -- both tables or the action
        half's alone -- so a rollout captured with `attended=False` never grows the entry by replaying."""
        from .model import decoder_params                        # (model imports this module)
        from .runtime import weight_key, ws_args
        if self.dtype != 'fp32' or not self.table.numel() or self.IMG % 4 or self.LOC % 16:
            return None
        hit = self._gate_rows.get(decoder)
        if hit is None and not build:
            return None
        w_ih = decoder_params(decoder)[0]
        key = weight_key(w_ih) + (self.table.data_ptr(), self.table._version)
        H = decoder.hidden_size
        attended = bool(attended) and H % 4 == 0 and bool(_lib.lib.sf_gate_rows_attended_supported(H, self.LOC))
        late = hit is not None and attended and hit['attended'] is None       # (asked for behind a build without it)
        if hit is None or hit['key'] != key or (late and build):
            if H % 4 or decoder.feature_size != self.F or tuple(w_ih.shape) != (4 * H, 2 * self.F):
                return None
            rows = self.n * self.V
            new = lambda r: torch.empty(r, 4 * H, device=self.device, dtype=torch.float32)  # noqa: E731
            same = hit is not None and hit['bufs'][0].shape == (rows, 4 * H)
            bufs = hit['bufs'] if same else (new(rows), new(4))
            call('sf_gate_rows_build', ptr(w_ih), ptr(self.table), rows, self.IMG, self.LOC, H, ptr(bufs[0]), ptr(bufs[1]),
                 *ws_args(self.device))
            struct = _lib.GateRows(bufs[0].data_ptr(), bufs[1].data_ptr(), w_ih.data_ptr(), H, self.V, self.IMG, self.LOC)
            att = hit['attended'] if same else None
            had = hit is not None and hit['attended'] is not None       # (a re-shaped table re-allocates what there was)
            if had or (attended and build):
                gf = att['buf'] if att is not None else new(rows)
                call('sf_gate_rows_attended_build', ptr(w_ih), ptr(self.table), rows, self.IMG, self.LOC, H, ptr(gf),
                     *ws_args(self.device))
                att = dict(buf=gf, struct=_lib.GateRowsAttended(gf.data_ptr(), w_ih.data_ptr(), H, self.V, self.IMG,
                                                                self.LOC))
            first = hit is None
            hit = dict(key=key, bufs=bufs, struct=struct, attended=att, builds=(0 if first else hit['builds']) + 1)
            self._gate_rows[decoder] = hit
            if first:
                addr = self.table.data_ptr()
                weakref.finalize(decoder, _forget_gate_rows, addr, bufs[0].data_ptr())
                weakref.finalize(self, _forget_gate_rows, addr, None)
        call('sf_gate_rows_register', C.c_void_p(self.table.data_ptr()), C.byref(hit['struct']))
        call('sf_gate_rows_attended_register', C.c_void_p(self.table.data_ptr()),
             C.byref(hit['attended']['struct']) if hit['attended'] is not None else None)
        return hit

    def note_unprojected(self, decoder):
        """An inference rollout of (this store, `decoder`) has just run WITHOUT projected tables under the 'auto' policy.
        From then on 'auto' leaves the pair alone (`seen_unprojected`): a rollout captured later replays the bits of the
        eager rollouts made before it, as it always did; `project = True` still builds."""
        if decoder not in self._projected:
            self._projected[decoder] = None

    def seen_unprojected(self, decoder):
        return decoder in self._projected and self._projected[decoder] is None

    # ---- pointer structs for the C ABI (tensors must stay alive while the call is enqueued) -----
    def pano(self, vp, view):
        return _lib.Pano(None, self.table.data_ptr(), self.loc_table.data_ptr(), vp.data_ptr(),
                         view.data_ptr(), self.V, self.IMG, self.LOC)

    def cands(self, vp, cand_view, sincos, a_num, A):
        return _lib.Cands(None, self.table.data_ptr(), vp.data_ptr(), cand_view.data_ptr(),
                          sincos.data_ptr(), a_num.data_ptr(), A, self.V, self.IMG, self.LOC)

    # ---- dense materialisation (what the reference agent feeds the modules) ---------------------
    def gather_panorama(self, vp, view):
        """[B,V,F] = features || location embedding (follower.py:291-298)."""
        B = vp.shape[0]
        out = torch.empty(B, self.V, self.F, device=self.device, dtype=torch.float32)
        p = self.pano(vp, view)
        call('sf_gather_panorama', C.byref(p), B, ptr(out), stream())
        return out

    def gather_candidates(self, vp, cand_view, sincos, a_num):
        """all_u_t [B,A,F], is_valid [B,A] (follower.py:300-320)."""
        B, A = cand_view.shape
        all_u = torch.empty(B, A, self.F, device=self.device, dtype=torch.float32)
        is_valid = torch.empty(B, A, device=self.device, dtype=torch.float32)
        c = self.cands(vp, cand_view, sincos, a_num, A)
        call('sf_gather_candidates', C.byref(c), B, ptr(all_u), ptr(is_valid), stream())
        return all_u, is_valid

    def gather_actions(self, vp, act_view, sincos, act):
        """[B,F] embeddings of one chosen action per sample (speaker.py:104); act <= 0 or
        vp < 0 gives zeros.  act_view/sincos are [B,1]-shaped candidate lists."""
        B = vp.shape[0]
        out = torch.empty(B, self.F, device=self.device, dtype=torch.float32)
        a_num = torch.full((B,), 2, dtype=torch.int32, device=self.device)
        cv = torch.stack((torch.zeros_like(act_view), act_view), 1).contiguous()
        sc = torch.stack((torch.zeros_like(sincos), sincos), 1).contiguous()
        c = self.cands(vp, cv, sc, a_num, 2)
        call('sf_gather_actions', C.byref(c), B, ptr(act), ptr(out), stream())
        return out
