"""Augmentation routes (data_augmentation_from_speaker.py; tasks/R2R/data/download_precomputed_augmentation.sh) made
here instead of downloaded, and handed to the speaker's sweep without a trip through the host per minibatch.

A route is a pure function of (start state, goal): the teacher's walk over the navigation tables.  `RouteSet` holds
N of them as arrays -- start row and view, goal row, and where the goal's row of the shared next-hop table
(`NavTable.all_hops`) starts -- from one of

  * `RouteSet.enumerate(nav, distances)`  every ordered (start, goal) pair of the chosen scans whose hop chain has
                                          min_hops .. max_hops edges and whose shortest distance is >= min_metres (R2R's
                                          rule, Anderson et al. 2018: 4 .. 6 edges, >= 5 m), ordered by scan, start row,
                                          goal row; start headings k * 30 degrees, k drawn from `seed`;
  * `RouteSet.from_items(nav, items)`     an existing split: start pose as NavTable.start_states snaps it, goal path[-1],
                                          the items' instr_encoding;
  * `.sample(n, seed)`                    a subset without replacement.

`.items()` / `.write_split(path)` give the R2R-format split, `.pack(B, Lmax)` the split's packed speaker minibatches
on the device: one sf_nav_routes launch for the lengths, one host sync, one launch per chunk of minibatches for the
blocks (csrc/sf_nav.hip; the layout is speaker.packed_layout's).  `speaker.SpeakerSweep.issue` takes the result in
place of host batches; `Seq2SeqSpeaker.augment(routes)` decodes it and `.replaced_items(results)` is the file
data_augmentation_from_speaker.py writes.

The follower's side (train.py --use_pretraining on the generated split): `.with_generated(results)` is the set with the
speaker's words as its instructions, `.pack_follower(B, Lmax, order)` its follower minibatches -- sorted by instruction
length, padded and laid out as nav.DeviceNavBatch.pack_layout -- written on the device by sf_nav_follower_batches, and
`Seq2SeqAgent.train_on_routes(routes, ...)` replays its training iterations over them with one device copy each.
`.follower_minibatch_host` is the same minibatch formed on the host, `.epoch_order` the default order of the draws."""
import copy
import ctypes as C
import json

import numpy as np
import torch

from . import _lib
from .env import ANGLE_INC
from .nav import V
from .runtime import stream
from .speaker import PackedBlocks, packed_layout
from .synth import EOS, PAD

PACK_CHUNK = 256       # minibatches per device buffer of `pack` (B = 100, Lmax = 80, Tp = 7: 87 104 bytes each, 22 MB)


class RouteSet:
    def __init__(self, nav, scan_ix, row0, view0, goal, heading, enc=None, path_ids=None, items=None):
        self.nav = nav
        self.scan_ix = np.asarray(scan_ix, np.int32)
        self.row0, self.view0, self.goal = (np.asarray(a, np.int32) for a in (row0, view0, goal))
        self.heading = np.asarray(heading, np.float64)
        self.enc = enc                                   # per route its token ids, or None: empty instructions
        self.path_ids = np.arange(len(self.row0)) if path_ids is None else np.asarray(path_ids)
        self.source_items = items                        # from_items: the split's own dictionaries
        self.distance = None                             # enumerate: D[start][goal]
        self.walked = None                               # enumerate: (n_actions, rows [S+1, N]) of the host walk
        self.unreached = 0                               # enumerate: pairs dropped because the teacher's walk did not arrive
        nav.all_hops()
        m = np.array([nav.scan_rows[s] for s in nav.scans], np.int64)
        base = np.array([nav.base[s] for s in nav.scans], np.int64)
        off = np.array([nav.hop_off[s] for s in nav.scans], np.int64)
        ix = self.scan_ix
        self.hop_base, self.hop_rows = base[ix].astype(np.int32), m[ix].astype(np.int32)
        self.hop_off = off[ix] + (self.goal - base[ix]) * m[ix]
        self._dev = None                                 # the device arrays, tokens among them (_device_arrays)
        self._tok = None                                 # the flat host token table (_host_tokens)
        self._route_dev = None                           # with_instructions: the route arrays of the set it copied
        # (`enc` is read once into `_tok` / `_dev`: another set of instructions is another set, `with_instructions`)

    def __len__(self):
        return len(self.row0)

    # ---- constructors
    @classmethod
    def enumerate(cls, nav, distances, scans=None, min_hops=4, max_hops=6, min_metres=5.0, seed=0):
        hop = nav.all_hops()
        parts = []
        for si, s in enumerate(nav.scans):
            if scans is not None and s not in scans:
                continue
            m, b, o = nav.scan_rows[s], nav.base[s], nav.hop_off[s]
            if distances.nodes[s] != [v for _, v in nav.vp_of[b:b + m]]:
                raise ValueError('the distance table and the navigation table order scan %s differently' % s)
            H = hop[o:o + m * m].reshape(m, m) - b                       # [goal, row] -> local next row
            G = np.arange(m)[:, None].repeat(m, 1)
            cur = np.arange(m)[None, :].repeat(m, 0)
            hops = np.full((m, m), -1, np.int64)                         # edges of the chain, -1: not within max_hops
            for t in range(max_hops + 1):
                arrived = (cur == G) & (hops < 0)
                hops[arrived] = t
                cur = H[G, cur]
            ok = (hops >= min_hops) & (hops <= max_hops) & (distances.block(s).T >= min_metres)   # [goal, start]
            start, goal = np.nonzero(ok.T)
            parts.append((np.full(len(start), si), start + b, goal + b, distances.block(s)[start, goal]))
        cat = lambda k, dt: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
        scan_ix, row0, goal, dist = cat(0, np.int32), cat(1, np.int32), cat(2, np.int32), cat(3, np.float64)
        k = np.random.default_rng(seed).integers(12, size=len(row0))
        out = cls(nav, scan_ix, row0, 12 + k, goal, k * ANGLE_INC)
        out.distance = dist
        n, reached, rows = out.walk_host(max_hops + 1)
        out.walked = (n, rows)
        if not reached.all():                                            # (the walk is the authority, not the chain)
            keep = np.flatnonzero(reached)
            kept = out.take(keep)
            kept.path_ids = np.arange(len(keep))
            kept.unreached = len(row0) - len(keep)
            return kept
        return out

    @classmethod
    def from_items(cls, nav, items):
        items = list(items)
        rows, views = nav.start_states(items)
        scan_of = {s: i for i, s in enumerate(nav.scans)}
        return cls(nav, [scan_of[it['scan']] for it in items], rows, views,
                   [nav.row_of[(it['scan'], it['path'][-1])] for it in items], [it['heading'] for it in items],
                   enc=[np.asarray(it['instr_encoding'], np.int64) for it in items],
                   path_ids=[it.get('path_id', i) for i, it in enumerate(items)], items=items)

    def take(self, idx):
        idx = np.asarray(idx, np.int64)
        out = RouteSet(self.nav, self.scan_ix[idx], self.row0[idx], self.view0[idx], self.goal[idx], self.heading[idx],
                       enc=None if self.enc is None else [self.enc[i] for i in idx], path_ids=self.path_ids[idx],
                       items=None if self.source_items is None else [self.source_items[i] for i in idx])
        if self.distance is not None:
            out.distance = self.distance[idx]
        if self.walked is not None:
            out.walked = (self.walked[0][idx], self.walked[1][:, idx])
        return out

    def sample(self, n, seed):
        """n distinct routes: default_rng(seed).permutation(len)[:n], in that order."""
        if n > len(self):
            raise ValueError('sample of %d from %d routes' % (n, len(self)))
        return self.take(np.random.default_rng(seed).permutation(len(self))[:n])

    # ---- the walk on the host (what sf_nav_routes' lengths mode leaves; NavTable.gold_routes' rules)
    def walk_host(self, S):
        """(n_actions [N] int32, reached [N] bool, rows [S+1, N] int32) of the teacher's walk, at most S actions."""
        h, hop = self.nav.host, self.nav.all_hops()
        N = len(self)
        row, view = self.row0.astype(np.int64), self.view0.astype(np.int64)
        cols = np.arange(h['next_row'].shape[1])[None, :]
        alive, stopped = np.ones(N, bool), np.zeros(N, bool)
        n, rows = np.zeros(N, np.int32), np.empty((S + 1, N), np.int32)
        rows[0] = row
        for t in range(S):
            s = row * V + view
            towards = hop[self.hop_off + (row - self.hop_base)]
            nxt = h['next_row'][s]
            leads = (nxt == towards[:, None]) & (cols >= 1) & (cols < h['a_num'][s][:, None])
            a = np.where((towards != row) & leads.any(1), leads.argmax(1), 0)
            n += alive
            stopped |= alive & (a == 0)
            go = alive & (a > 0) & (nxt[np.arange(N), a] != row)
            view = np.where(go, h['cand_view'][s, a], view)
            row = np.where(go, nxt[np.arange(N), a], row)
            alive &= a > 0
            rows[t + 1] = row
        return n, stopped & (row == self.goal), rows

    # ---- the split in R2R's format
    @property
    def instr_ids(self):
        if self.source_items is not None:
            return [it['instr_id'] for it in self.source_items]
        return ['%d_0' % p for p in self.path_ids]

    def items(self, first_path_id=0, S=10):
        """R2R-format dictionaries (an existing split: its own items): path_id, scan, heading, path (the viewpoints of
        the walked rows; a set that was not enumerated is walked here, at most S actions), distance,
        instructions [''], instr_id '<path_id>_0' and an empty instr_encoding."""
        if self.source_items is not None:
            return list(self.source_items)
        if self.walked is None:
            self.walked = self.walk_host(S)[::2]
        n, rows = self.walked
        vp_of, scans = self.nav.vp_of, self.nav.scans
        out = []
        for i in range(len(self)):
            pid = first_path_id + int(self.path_ids[i])
            out.append(dict(path_id=pid, scan=scans[self.scan_ix[i]], heading=float(self.heading[i]),
                            path=[vp_of[r][1] for r in rows[:n[i], i]],
                            distance=float(self.distance[i]) if self.distance is not None else 0.0, instructions=[''],
                            instr_id='%d_0' % pid, instr_encoding=[]))
        return out

    def write_split(self, path, first_path_id=0):
        with open(path, 'w') as f:
            json.dump(self.items(first_path_id), f)

    def replaced_items(self, results, tokenizer=None, first_path_id=0):
        """What SpeakerEvaluation.score_results returns beside the summary (eval_speaker.py:83-85) and
        data_augmentation_from_speaker.py writes: per path, in path_id order, the item with instructions =
        [' '.join(words)] of the first result of that path.  tokenizer: decodes 'word_indices' where a result has no
        'words'."""
        by_path = {}
        for it in self.items(first_path_id):
            by_path.setdefault(it['path_id'], it)
        first = {}
        for instr_id, result in results.items():
            first.setdefault(int(instr_id.split('_')[0]), result)
        out = []
        for pid, result in sorted(first.items()):
            if pid not in by_path:
                continue
            words = result['words'] if tokenizer is None else tokenizer.decode_sentence(
                result['word_indices'], break_on_eos=True, join=False)
            item = by_path[pid].copy()
            item['instructions'] = [' '.join(str(w) for w in words)]
            out.append(item)
        return out

    # ---- on the device
    def _host_tokens(self):
        """(flat int64 token ids of every route end to end, one spare element behind; instr_off [N+1] int64)."""
        if self._tok is None:
            enc = self.enc if self.enc is not None else [()] * len(self)
            off = np.concatenate(([0], np.cumsum([len(e) for e in enc]))).astype(np.int64)
            flat = np.concatenate([np.asarray(e, np.int64).reshape(-1) for e in enc] + [np.zeros(1, np.int64)])
            self._tok = (flat, off)
        return self._tok

    def _device_arrays(self):
        if self._dev is None:
            dev = self.nav.device
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)             # noqa: E731
            shared = self._route_dev
            d = dict(shared) if shared is not None else dict(
                row0=up(self.row0, np.int32), view0=up(self.view0, np.int32), goal=up(self.goal, np.int32),
                hop_off=up(self.hop_off, np.int64), hop_base=up(self.hop_base, np.int32),
                hop_rows=up(self.hop_rows, np.int32), hop_all=self.nav.all_hops_device())
            d['tokens'] = d['instr_off'] = None
            if self.enc is not None:
                flat, off = self._host_tokens()
                d['tokens'], d['instr_off'] = up(flat, np.int64), up(off, np.int64)
            self._dev = d
        return self._dev

    def _io(self, S, n_slots, **kw):
        d = self._device_arrays()
        p = lambda t: None if t is None else t.data_ptr()                                        # noqa: E731
        f = dict(N=len(self), S=int(S), n_slots=int(n_slots), B=0, Lmax=0, M=0, pad=PAD, eos=EOS, row0=p(d['row0']),
                 view0=p(d['view0']), goal=p(d['goal']), hop_all=p(d['hop_all']), hop_off=p(d['hop_off']),
                 hop_base=p(d['hop_base']), hop_rows=p(d['hop_rows']))
        f.update(kw)
        return _lib.NavRoutesIO(**f)

    def lengths(self, S):
        """ONE sf_nav_routes launch in lengths mode on the current stream: the device tensors n_actions, reached [N],
        rows [S+1, N] (int32) and err [1], not waited for."""
        dev, N = self.nav.device, len(self)
        out = dict(n_actions=torch.empty(N, dtype=torch.int32, device=dev), reached=torch.empty(N, dtype=torch.int32, device=dev),
                   rows=torch.empty(S + 1, N, dtype=torch.int32, device=dev), err=torch.zeros(1, dtype=torch.int32, device=dev))
        io = self._io(S, N, n_actions=out['n_actions'].data_ptr(), reached=out['reached'].data_ptr(), rows=out['rows'].data_ptr())
        _lib.call('sf_nav_routes', C.byref(self.nav.struct()), C.byref(io), C.c_void_p(out['err'].data_ptr()), stream())
        return out

    def pack(self, B, Lmax, chunk=None, S=10):
        """The split as packed speaker minibatches of B routes on the device (speaker.PackedBlocks): a lengths launch, ONE
        host sync (the step count Tp of a minibatch is its longest route: the speaker's path encoder does not mask by
        length, so Tp must be what the host path would use), then one pack launch per `chunk` minibatches, each into
        its own uint8 buffer.  A last minibatch short of B is filled with routes from the front (index i mod N), as
        the environment fills it.  S: most actions of a route (the agent's max_episode_len)."""
        N, dev = len(self), self.nav.device
        if N < 1:
            raise ValueError('no routes to pack')
        first = self.lengths(S)
        n = first['n_actions'].cpu().numpy()                                 # the one host sync
        if int(first['err'].item()):
            raise RuntimeError('sf_nav_routes: a start state outside the navigation table')
        M = -(-N // B)
        route = (np.arange(M * B) % N).astype(np.int32)
        Tp = n[route].reshape(M, B).max(1).astype(np.int32)
        nbytes = np.array([packed_layout(B, int(t), Lmax)['bytes'] for t in Tp], np.int64)
        chunk = int(chunk or PACK_CHUNK)
        d = self._device_arrays()
        route_dev, Tp_dev = torch.from_numpy(route).to(dev), torch.from_numpy(Tp).to(dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        blocks, keep = [], [d, route_dev, Tp_dev]
        for lo in range(0, M, chunk):
            hi = min(M, lo + chunk)
            off = np.concatenate(([0], np.cumsum(nbytes[lo:hi]))).astype(np.int64)
            buf = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
            off_dev = torch.from_numpy(off[:-1].copy()).to(dev)
            Tp_host, off_host = np.ascontiguousarray(Tp[lo:hi]), np.ascontiguousarray(off[:-1])
            io = self._io(S, (hi - lo) * B, B=B, Lmax=Lmax, M=hi - lo, route=route_dev[lo * B:].data_ptr(),
                          mb_Tp=Tp_host.ctypes.data, mb_off=off_host.ctypes.data, mb_Tp_dev=Tp_dev[lo:].data_ptr(),
                          mb_off_dev=off_dev.data_ptr(), instr_tokens=None if d['tokens'] is None else d['tokens'].data_ptr(),
                          instr_off=None if d['instr_off'] is None else d['instr_off'].data_ptr(), out=buf.data_ptr(),
                          out_bytes=buf.numel())
            _lib.call('sf_nav_routes', C.byref(self.nav.struct()), C.byref(io), C.c_void_p(err.data_ptr()), stream())
            blocks += [(buf, int(off[i]), int(Tp[lo + i])) for i in range(hi - lo)]
            keep.append(off_dev)
        return PackedBlocks(blocks, B, Lmax, err=err, keep=keep, n_actions=n, route=route)

    # ---- the follower's side: pre-training on the set (train.py --use_pretraining), minibatches packed on the device
    def with_instructions(self, enc):
        """A copy of the set whose instructions are `enc`: per route its token ids.  The routes, and their device
        arrays where they exist, are shared; the device token arrays are rebuilt when next needed."""
        enc = [np.asarray(e, np.int64).reshape(-1) for e in enc]
        if len(enc) != len(self):
            raise ValueError('%d instructions for %d routes' % (len(enc), len(self)))
        out = copy.copy(self)
        out.enc, out._tok, out._dev = enc, None, None
        if self._dev is not None or self._route_dev is not None:
            src = self._dev if self._dev is not None else self._route_dev
            out._route_dev = {k: v for k, v in src.items() if k not in ('tokens', 'instr_off')}
        return out

    def with_generated(self, results, tokenizer=None):
        """`with_instructions` of what `Seq2SeqSpeaker.augment(self)` returned: per route (by `instr_ids`) the result's
        'word_indices' up to, not including, the first EOS -- the cut of decode_sentence(break_on_eos=True).  The
        vocabulary ids are used as they are.  The reference writes the words joined into a string and re-tokenises
        that string when the split is loaded; the two differ only for an id whose text does not encode back to the id
        itself (<UNK>, <BOS>, <PAD>).  With a `tokenizer` (decode_sentence / encode_sentence) returns (set, number of
        routes holding such an id), else the set."""
        enc = []
        for key in self.instr_ids:
            w = np.asarray(results[key]['word_indices'], np.int64).reshape(-1)
            stop = np.flatnonzero(w == EOS)
            enc.append(w[:stop[0]] if len(stop) else w)
        out = self.with_instructions(enc)
        if tokenizer is None:
            return out
        ids = np.unique(np.concatenate(enc)) if enc else np.zeros(0, np.int64)
        back = lambda v: [int(x) for x in tokenizer.encode_sentence(                             # noqa: E731
            tokenizer.decode_sentence([int(v)], break_on_eos=True, join=True))[0]]
        odd = np.array([v for v in ids if back(v) != [int(v)]], np.int64)
        return out, sum(1 for e in enc if np.isin(e, odd).any())

    def follower_minibatch_host(self, idx, Lmax, reverse=True):
        """The follower minibatch that draws the routes `idx` (in that order), formed on the host from the set's arrays
        and NavTable.all_hops: what env._next_minibatch(sort=True) + DeviceNavBatch.host_arrays_for(..., fixed=True)
        form from item dictionaries -- columns by token count descending, equal counts in draw order; seq [B, Lmax]
        int64 (tokens, last first when `reverse`, then EOS, cut to Lmax, PAD behind), mask uint8 (seq == PAD), lengths,
        rows, views, hop [B, largest scan] (zeros behind a smaller scan's rows), base -- plus 'route': idx as sorted.
        The contract sf_nav_follower_batches is held to, and the minibatch a capturing iteration is built from."""
        idx = np.asarray(idx, np.int64).reshape(-1)
        flat, off = self._host_tokens()
        raw = off[idx + 1] - off[idx]
        route = idx[np.argsort(-raw, kind='stable')]
        first, n = off[route], off[route + 1] - off[route]
        assert not ((n > 0) & (flat[first + n - 1] == EOS)).any(), 'an instruction that ends in EOS'
        k = np.arange(Lmax, dtype=np.int64)[None, :]
        src = first[:, None] + np.where(k < n[:, None], (n[:, None] - 1 - k) if reverse else k, 0)
        seq = np.where(k < n[:, None], flat[np.minimum(src, len(flat) - 1)], np.where(k == n[:, None], EOS, PAD)).astype(np.int64)
        hop_all, ld = self.nav.all_hops(), max(self.nav.scan_rows.values())
        m = self.hop_rows[route].astype(np.int64)
        c = np.arange(ld, dtype=np.int64)[None, :]
        live = c < m[:, None]
        hop = np.where(live, hop_all[self.hop_off[route][:, None] + np.where(live, c, 0)], 0).astype(np.int32)
        return dict(seq=np.ascontiguousarray(seq), mask=np.ascontiguousarray((seq == PAD).astype(np.uint8)),
                    lengths=np.minimum(n + 1, Lmax).astype(np.int32), rows=self.row0[route].copy(),
                    views=self.view0[route].copy(), hop=np.ascontiguousarray(hop), base=self.hop_base[route].copy(),
                    route=route)

    def epoch_order(self, B, n_minibatches, seed=0):
        """int32 [n_minibatches * B]: epoch e is default_rng([seed, e]).permutation(N); the epochs laid end to end and
        cut to length (a minibatch may straddle two epochs, as the environment's does)."""
        N, total = len(self), int(n_minibatches) * int(B)
        if N < 1:
            raise ValueError('no routes to order')
        epochs = [np.random.default_rng([seed, e]).permutation(N) for e in range(-(-total // N))]
        return np.concatenate(epochs + [np.zeros(0, np.int64)])[:total].astype(np.int32)

    def pack_follower(self, B, Lmax, order=None, reverse=True, chunk=None):
        """The set as follower minibatches of B routes on the device (nav.FollowerBlocks; the layout is
        DeviceNavBatch.pack_layout(B, Lmax, ld) with ld the largest scan of `nav`): one sf_nav_follower_batches launch per
        `chunk` minibatches, each into its own uint8 buffer, then ONE host sync that brings down err, col_route and
        col_len.  order: the route index of every slot, minibatch i draws slots i*B .. i*B + B - 1 (None: arange(M * B)
        % N, a short tail filled from the front as `pack` fills it)."""
        from .nav import DeviceNavBatch, FollowerBlocks
        N, dev = len(self), self.nav.device
        if N < 1:
            raise ValueError('no routes to pack')
        if order is None:
            order = np.arange(-(-N // B) * B) % N
        order = np.ascontiguousarray(order, np.int32).reshape(-1)
        if len(order) < B or len(order) % B:
            raise ValueError('an order of %d slots is not a whole number of minibatches of %d' % (len(order), B))
        M, ld = len(order) // B, max(self.nav.scan_rows.values())
        nbytes = DeviceNavBatch.pack_layout(B, Lmax, ld)['bytes']
        chunk = int(chunk or PACK_CHUNK)
        d = self._device_arrays()
        p = lambda t: None if t is None else t.data_ptr()                                        # noqa: E731
        order_dev = torch.from_numpy(order).to(dev)
        down = torch.zeros(1 + 2 * M * B, dtype=torch.int32, device=dev)     # err, col_route [M, B], col_len [M, B]
        blocks, keep = [], [d, order_dev]
        for lo in range(0, M, chunk):
            hi = min(M, lo + chunk)
            off = np.arange(hi - lo, dtype=np.int64) * nbytes
            buf = torch.empty((hi - lo) * nbytes, dtype=torch.uint8, device=dev)
            off_dev = torch.from_numpy(off).to(dev)
            io = _lib.NavFollowerIO(N=N, V=V, B=B, Lmax=Lmax, ld=ld, M=hi - lo, pad=PAD, eos=EOS, reverse=int(bool(reverse)),
                                    row0=p(d['row0']), view0=p(d['view0']), hop_all=p(d['hop_all']), hop_off=p(d['hop_off']),
                                    hop_base=p(d['hop_base']), hop_rows=p(d['hop_rows']), instr_tokens=p(d['tokens']),
                                    instr_off=p(d['instr_off']), order=p(order_dev[lo * B:]), mb_off=off.ctypes.data,
                                    mb_off_dev=p(off_dev), out=p(buf), out_bytes=buf.numel(),
                                    col_route=p(down[1 + lo * B:]), col_len=p(down[1 + (M + lo) * B:]))
            _lib.call('sf_nav_follower_batches', C.byref(io), C.c_void_p(down.data_ptr()), stream())
            blocks += [(buf, int(o)) for o in off]
            keep.append(off_dev)
        host = down.cpu().numpy()                                            # the one host sync
        if int(host[0]):
            raise RuntimeError('sf_nav_follower_batches refused a slot: a route index, a start view, a scan wider than '
                               'the hop columns, or an instruction that ends in EOS')
        return FollowerBlocks(blocks, B, Lmax, ld, col_route=host[1:1 + M * B].reshape(M, B),
                              col_len=host[1 + M * B:].reshape(M, B), keep=keep)

    def follower_windows(self, B, Lmax, order, reverse=True, window=None):
        """`pack_follower` of a long `order` a window at a time (FollowerWindows): what a training loop of many
        iterations draws its minibatches from without holding all of them on the device."""
        return FollowerWindows(self, B, Lmax, order, reverse, int(window or PACK_CHUNK))


class FollowerWindows:
    """The minibatches of `order` (route index of every slot, a whole number of minibatches of B), packed `window` of
    them per `RouteSet.pack_follower` call when the first of a window is asked for -- one launch and one host sync per
    window.  `at(i)` -> (nav.FollowerBlocks, index in it) for `DeviceNavBatch.load_packed`.  The window before the
    current one is kept (a training loop reloads the iteration still in flight when it faulted), older ones are dropped:
    at most 2 * window blocks are alive."""

    def __init__(self, routes, B, Lmax, order, reverse=True, window=PACK_CHUNK):
        order = np.ascontiguousarray(order, np.int32).reshape(-1)
        if len(order) < B or len(order) % B:
            raise ValueError('an order of %d slots is not a whole number of minibatches of %d' % (len(order), B))
        self.routes, self.B, self.Lmax, self.order, self.reverse, self.window = routes, B, Lmax, order, reverse, window
        self.packed = 0                                      # pack_follower calls so far
        self._alive = {}

    def __len__(self):
        return len(self.order) // self.B

    def at(self, i):
        w, B = i // self.window, self.B
        if w not in self._alive:
            for old in [k for k in self._alive if k != w - 1]:
                del self._alive[old]
            lo = w * self.window * B
            self._alive[w] = self.routes.pack_follower(B, self.Lmax, order=self.order[lo:lo + self.window * B],
                                                       reverse=self.reverse)
            self.packed += 1
        return self._alive[w], i - w * self.window
