"""Search procedures of the follower and the speaker on the HIP path:

* `beam_search`            -- Seq2SeqAgent.beam_search            (follower.py:541-718)
* `state_factored_search`  -- Seq2SeqAgent.state_factored_search  (follower.py:720-980)
* `speaker_beam_search`    -- Seq2SeqSpeaker.beam_search          (speaker.py:211-318)
* `rational_mix`, `run_rational_follower` -- the pragmatic re-ranking (rational_follower.py:12-190)

The three searches live in frontier.py: hypotheses are rows of integer / float32 arrays with parent pointers,
world states are integers into the navigation tables (nav.NavTable), the per-instance bookkeeping is numpy over
the whole minibatch.  This module holds what they share with the rest of the package: the flat decoder steps
on the device, the helpers the reference exports from follower.py (`least_common_viewpoint_path`,
`backchain_inference_states`, `InferenceState`) and the re-ranking.  Every iteration is ONE flat decoder
step over all live states on the device:

  reference (per iteration)                            here
  -----------------------------------------------     ------------------------------------------------
  np.stack of N x 36 x 2176 features + H2D             N x (row, view) int32 -> kernels gather from HBM
  all_u_t [N,A,2176] built on the host + H2D           N x A (view, sin/cos) -> gathered in the kernel
  h_t[flat_indices], c_t[flat_indices]                 sf_gather_rows from the state pool
  ctx[beam_indices], seq_mask[beam_indices] (copies)   ctx_row indirection inside the attention kernel
  log_softmax + topk + gather, .data on the host       sf_logprob_topk, one D2H of [N,k] per iteration
  last_action_embedding = all_u_t[i, a] (2176 floats)  (row, view, sin/cos) of the parent's table entry
  env.step / env.observe per successor (Python)        next_row[s, a], cand_view[s, a] look-ups (numpy)

The agent needs a `features.FeatureStore` (`agent.store`) and an env.R2RIndexEnv.
"""
import ctypes as C
import time
from collections import namedtuple, Counter

import numpy as np
import torch

from . import _lib
from ._lib import call
from .features import cand_sincos
from .follower import batch_instructions_from_encoded, EOS, BOS
from .frontier import SEARCH_NODE_FIELDS
from .model import decoder_params, decoder_w_struct, decoder_tape, tape_struct
from .runtime import ptr, stream, ws_args, gc_paused, graph_capture, ensure_workspace, check_gate_weights, gate_weights_pass, register_bf16_weights, gate_mode_key

byref = C.byref

# follower.py:19 -- h_t / c_t / last_alpha hold rows of the device state pool instead of tensors,
# last_action_embedding holds the index-form descriptor of the embedding instead of 2176 floats
InferenceState = namedtuple(
    'InferenceState',
    'prev_inference_state, world_state, observation, flat_index, last_action, '
    'last_action_embedding, action_count, score, h_t, c_t, last_alpha')

SpeakerInferenceState = namedtuple(
    'SpeakerInferenceState',
    'prev_inference_state, flat_index, last_word, word_count, score, last_alpha')   # speaker.py:18

def _add_f32(score, step_score):
    """The reference accumulates hypothesis scores as `score + action_score` with action_score a
    float32 tensor element (follower.py:629, 826; speaker.py:277): every partial sum is rounded to
    float32.  Same rounding here, so that ties and orderings agree."""
    return float(np.float32(score) + np.float32(step_score))


def flatten(lol):
    return [x for l in lol for x in l]                                               # utils.py:205


def path_element_from_observation(ob):
    return (ob['viewpoint'], ob['heading'], ob['elevation'])


def _lineage(inf_state):
    """The state and its ancestors, newest first (back-pointer chain of InferenceState)."""
    chain = []
    while inf_state is not None:
        chain.append(inf_state)
        inf_state = inf_state.prev_inference_state
    return chain


def backchain_inference_states(last_inference_state):
    """What follower.py:33-50 returns for a hypothesis: (world states, observations, actions,
    per-action scores, attention rows), oldest first; the start pseudo-action (and its attention
    row) is left out, and the score of action i is the difference of the cumulative scores on
    either side of it."""
    chain = _lineage(last_inference_state)[::-1]
    taken = chain[1:]
    return ([s.world_state for s in chain], [s.observation for s in chain],
            [s.last_action for s in taken],
            [s.score - p.score for p, s in zip(chain, taken)],
            [s.last_alpha for s in taken])


def least_common_viewpoint_path(inf_state_a, inf_state_b):
    """The physical walk between two frontier states (follower.py:52-73): up from A to its nearest
    ancestor standing on a viewpoint that B's lineage also visits, then down B's lineage from the
    OLDEST state on that viewpoint to B.  The meeting viewpoint appears once."""
    down = _lineage(inf_state_b)                       # B, parent(B), ..., root
    oldest_at = {s.world_state.viewpointId: i for i, s in enumerate(down)}   # later (older) index wins
    up = []
    for s in _lineage(inf_state_a):
        up.append(s)
        i = oldest_at.get(s.world_state.viewpointId)
        if i is not None:
            return up + down[:i][::-1]
    raise AssertionError('the two states share no viewpoint on their lineages')


class _Pool:
    """Rows of per-state device data that outlive the iteration that produced them (hidden and
    cell state, text attention).  Decoder steps write straight into the next free rows."""

    def __init__(self, width, device, cap=256):
        self.buf = torch.empty(cap, width, device=device, dtype=torch.float32)
        self.n = 0

    def reserve(self, n):
        if self.n + n > self.buf.shape[0]:
            cap = max(2 * self.buf.shape[0], self.n + n)
            new = torch.empty(cap, self.buf.shape[1], device=self.buf.device, dtype=torch.float32)
            new[:self.n].copy_(self.buf[:self.n])
            self.buf = new
        base = self.n
        self.n += n
        return base, self.buf[base:base + n]


def _gate_pass(obj):
    """The gate-product mode `obj` (a decoder-step object with .dec and .gate_weights) issues its inference steps under."""
    return gate_weights_pass(obj.gate_weights, obj.dec.lstm.weight_ih, obj.dec.lstm.weight_hh)


def _baked_weights(obj):
    """The weight-side pointers a captured step of `obj` bakes (stale cached layouts are refreshed in place): the decoder
    struct and, with gate_weights = 'bf16', the packed images of the LSTM weights."""
    wb = bytes(decoder_w_struct(decoder_params(obj.dec)))
    if obj.gate_weights == 'bf16':
        wb += repr(tuple(t.data_ptr() for t in register_bf16_weights(obj.dec.lstm.weight_ih, obj.dec.lstm.weight_hh))).encode()
    return wb


class _DeviceLoop:
    """What the searches with their steps on the device share (GraphStep, DeviceStateFactored, DeviceSpeakerBeam,
    DeviceFollowerBeam): the capture of a chunk of steps as one hipGraph, the replay-or-issue chunk loop and the
    counters of its host reads.  A subclass has `dev`, `chunk` and `_issue_steps(n)`, which issues n steps on the
    current stream."""
    _side = None                                          # the capture stream: ONE per object, for its lifetime
    captures = 0
    host_reads = last_host_reads = minibatches = 0
    last_run_s = 0.0                                      # (the step loop and its download, seconds)

    def _capture_steps(self, n_steps, graphs=True):
        """`n_steps` steps as one hipGraph (graphs = False: 'eager', nothing captured), after one eager warm-up step
        (cached layouts, lazy tables).  The caller has put the buffers into a state in which a step changes nothing.
        Every capture of the object runs on its one side stream: a graph bakes that stream's workspace, and a stream
        per capture would leave one workspace behind per re-capture (runtime._workspaces)."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        side = self._side
        ensure_workspace(side, self.dev)                  # (before the capture: runtime.workspace)
        side.wait_stream(torch.cuda.current_stream())
        graph = 'eager'
        with torch.no_grad(), torch.cuda.stream(side):
            self._issue_steps(1)
            side.synchronize()
            if graphs:
                graph = torch.cuda.CUDAGraph()
                with graph_capture(graph, side):
                    self._issue_steps(n_steps)
        torch.cuda.current_stream().wait_stream(side)
        self.captures += 1
        return graph

    def _step_chunk(self, graph):
        """One chunk of steps: the captured graph's replay, or (graph None / 'eager') issued launch by launch."""
        if graph is None or graph == 'eager':
            self._issue_steps(self.chunk)
        else:
            graph.replay()

    def _run_chunks(self, graph, limit, live_total):
        """Chunks until `limit` steps are issued or the chunk's last step left nothing live (live_total: the device
        array of the live count after every step; one 4-byte read per chunk).  Returns (steps to download, reads)."""
        reads = issued = 0
        while issued < limit:
            self._step_chunk(graph)
            issued += self.chunk
            if issued >= limit:
                break
            reads += 1
            if int(live_total[issued - 1].item()) == 0:
                break
        return min(issued, limit), reads

    def _count_run(self, reads, t0):
        self.last_host_reads = reads
        self.host_reads += reads
        self.minibatches += 1
        self.last_run_s = time.perf_counter() - t0


class BeamRecord:
    """The layout of a beam search's record, one int32 buffer downloaded once at the end (host arithmetic only):

        [inst B x 3 | live_total steps | done_rec B x 2 beam | done_score B x 2 beam], padded to 4 words, then per step
        [one plane of R = B * beam words per name in `planes` | attention R x width]

    The last of `planes` (the score) and the attention are float32, the rest int32."""

    def __init__(self, B, beam, steps, planes, width):
        self.B, self.beam, self.steps, self.planes, self.width = B, beam, steps, tuple(planes), width
        self.R = B * beam
        self.o_live = 3 * B
        self.o_done = self.o_live + steps
        self.o_dscore = self.o_done + 2 * beam * B
        self.hdr = (self.o_dscore + 2 * beam * B + 3) & ~3
        self.stride = self.R * (len(self.planes) + width)
        self.size = self.hdr + steps * self.stride

    def head0(self):
        """The header at the start of a search: one live slot per instance, nothing done, t = 0."""
        head = np.zeros(self.hdr, np.int32)
        head[0:3 * self.B:3] = 1
        return head

    def pointers(self, base):
        """(inst, live_total, one pointer per plane, attention, ld_hist, done_rec, done_score) of a record at device
        address `base`: the tail of the SpkBeam / FolBeam constructors."""
        steps = base + 4 * self.hdr
        return (base, base + 4 * self.o_live, *(steps + 4 * j * self.R for j in range(len(self.planes) + 1)),
                self.stride, base + 4 * self.o_done, base + 4 * self.o_dscore)

    def split(self, flat, attn='attn'):
        """A downloaded record (int32, header and at least the steps that ran) as host arrays: inst [B,3], done_rec /
        done_score [B, 2 beam], every plane [t_end, R] under its name, the attention [t_end, R, width] under `attn`;
        t_end: the step after the last one any instance ran."""
        B, R, W2 = self.B, self.R, 2 * self.beam
        inst = flat[:3 * B].reshape(B, 3)
        t_end = int(inst[:, 2].max())
        fl = flat.view(np.float32)
        st = flat[self.hdr:self.hdr + t_end * self.stride].reshape(t_end, self.stride)
        stf = fl[self.hdr:self.hdr + t_end * self.stride].reshape(t_end, self.stride)
        out = dict(inst=inst, done_rec=flat[self.o_done:self.o_dscore].reshape(B, W2),
                   done_score=fl[self.o_dscore:self.o_dscore + W2 * B].reshape(B, W2))
        n = len(self.planes)
        for j, name in enumerate(self.planes):
            out[name] = (stf if j == n - 1 else st)[:, j * R:(j + 1) * R]
        out[attn] = stf[:, n * R:].reshape(t_end, R, self.width)
        return out


def _owner_cache(owner, name, key, limit, build, **same):
    """The object `owner` keeps under `key` in its dictionary `name` (buffers and captured graphs; built on first use).
    `same`: attributes of the kept object that must still BE these objects (a key holds ids, and an id can come back
    on another object).  A cache of `limit` entries is emptied before one more goes in."""
    cache = owner.__dict__.setdefault(name, {})
    obj = cache.get(key)
    if obj is None or any(getattr(obj, a) is not v for a, v in same.items()):
        if len(cache) >= limit:
            cache.clear()
        obj = cache[key] = build()
    return obj


def _observation_buffers(n, A, dev):
    """Outputs of sf_nav_step over 2n states: the observations of n states [0] and of their parents [1] as halves of
    one [2n] look-up.  Returns (the whole block, its two halves)."""
    i32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int32)                 # noqa: E731
    obs2 = dict(row=i32(2 * n), vp=i32(2 * n), view=i32(2 * n), a_num=i32(2 * n), cand_view=i32(2 * n, A),
                sincos=torch.zeros(2 * n, A, 4, device=dev, dtype=torch.float32))
    return obs2, [{k: v[j * n:(j + 1) * n] for k, v in obs2.items()} for j in range(2)]


def _follower_steps(obj, n_steps, n, rows, views, act, hsrc, csrc, hrow, crow, k, idx, logp, then):
    """`n_steps` follower decode steps over the n fixed rows of `obj` (a GraphStep or a DeviceFollowerBeam: store, nav,
    dec, obs2 / obs, tape, h0 / c0, ctx / mask, H / D / T / A), per step

        sf_nav_step over the [2n] block (rows, views) -> obj.obs2; the previous action's embedding out of the parents'
        candidates straight into the first half of the LSTM input rows (sf_gather_actions_ld; action 0 = zeros =
        u_begin: no copy in the step); h0 / c0 = hsrc / csrc [hrow] (sf_move_rows); sf_attn_decoder_fwd with
        instruction rows `crow` under the object's gate-product mode; sf_logprob_topk (k columns, n_valid = a_num) ->
        idx (or None) / logp; then(stream): what the search does with them.

    Returns the pointer structs of the launches: the caller keeps them for as long as a captured graph may replay."""
    st, A, H = obj.store, obj.A, obj.H
    s = stream()
    o = obj.obs2
    cur, par = obj.obs
    ns = obj.nav.struct()
    ucand = st.cands(par['vp'], par['cand_view'], par['sincos'], par['a_num'], A)
    gat = (_lib.RowMove * 2)(_lib.RowMove(hsrc.data_ptr(), obj.h0.data_ptr(), hrow.data_ptr(), H, H, H, 0),
                             _lib.RowMove(csrc.data_ptr(), obj.c0.data_ptr(), hrow.data_ptr(), H, H, H, 0))
    pano = st.pano(cur['vp'], cur['view'])
    cnd = st.cands(cur['vp'], cur['cand_view'], cur['sincos'], cur['a_num'], A)
    w = decoder_w_struct(decoder_params(obj.dec))
    tp = tape_struct(obj.tape)
    for _ in range(n_steps):
        call('sf_nav_step', byref(ns), 2 * n, ptr(rows), ptr(views), None, None, None, 0, None,
             ptr(o['row']), ptr(o['vp']), ptr(o['view']), ptr(o['a_num']), ptr(o['cand_view']), ptr(o['sincos']), None, s)
        call('sf_gather_actions_ld', byref(ucand), n, ptr(act), ptr(obj.tape['xin']), 2 * st.F, s)
        call('sf_move_rows', gat, 2, n, s)
        with _gate_pass(obj):
            call('sf_attn_decoder_fwd', byref(w), byref(pano), byref(cnd), n, H, obj.D, obj.T,
                 None, ptr(obj.h0), ptr(obj.c0), ptr(obj.ctx), ptr(obj.mask), ptr(crow), byref(tp), None,
                 None, 0, *ws_args(obj.dev))
        call('sf_logprob_topk', ptr(obj.tape['logit']), A, n, A, ptr(cur['a_num']), k, ptr(idx), ptr(logp), s)
        then(s)
    return ns, ucand, pano, cnd, w, tp, gat


class FlatDecoder:
    """One follower decoder step over a flat list of search states (a6 without the glue).  `gate_weights`: 'fp32' or 'bf16'
    (FollowerEngine.gate_weights; steps of more than 128 states run the fp32-weight kernels in either mode)."""

    def __init__(self, decoder, store, ctx, mask, gate_weights='fp32'):
        self.gate_weights = check_gate_weights(gate_weights)
        self.dec, self.store = decoder, store
        self.ctx, self.mask = ctx.contiguous(), mask.to(torch.uint8).contiguous()
        self.dev = store.device
        self.H = decoder.hidden_size
        self.D = decoder.visual_attention_layer.linear_in_h.weight.shape[0]
        self.T = ctx.shape[1]
        self.hpool = _Pool(self.H, self.dev)
        self.cpool = _Pool(self.H, self.dev)
        self.apool = _Pool(self.T, self.dev)
        self.w = decoder_w_struct(decoder_params(decoder))
        self._keep = None

    def seed(self, h, c):
        """Encoder outputs become pool rows 0..B-1."""
        B = h.shape[0]
        _, hv = self.hpool.reserve(B)
        _, cv = self.cpool.reserve(B)
        self.apool.reserve(B)
        hv.copy_(h)
        cv.copy_(c)

    def step(self, flat_obs, u_desc, state_rows, beam_indices, k):
        """Dictionary-style front end of `step_arrays`: flat_obs = N index-form observations; u_desc = N
        descriptors (row, view, heading, elevation) of the previous action's embedding or None (u_begin = zeros,
        model.py:368); state_rows = pool rows of (h, c); beam_indices = instance of each state.  Returns (pool
        row base of the N new states, a_num [N], top-k columns [N,k] and their log-probabilities [N,k])."""
        N = len(flat_obs)
        a_num = np.array([len(ob['adj_loc_list']) for ob in flat_obs], np.int64)
        A = int(a_num.max())
        head, elev = np.zeros((N, A)), np.zeros((N, A))
        cview = np.zeros((N, A), np.int64)
        for i, ob in enumerate(flat_obs):
            for a_, d in enumerate(ob['adj_loc_list'][1:], 1):
                cview[i, a_], head[i, a_], elev[i, a_] = d['absViewIndex'], d['rel_heading'], d['rel_elevation']
        has_u = np.array([u is not None for u in u_desc])
        ud = [u if u is not None else (0, 0, 0.0, 0.0) for u in u_desc]
        inputs = dict(vp=np.array([ob['vp_row'] for ob in flat_obs]), view=np.array([ob['viewIndex'] for ob in flat_obs]),
                      a_num=a_num, cand_view=cview, sincos=cand_sincos(head, elev), hrow=np.asarray(state_rows),
                      crow=np.asarray(beam_indices), has_u=has_u, u_vp=np.array([u[0] for u in ud]),
                      u_view=np.array([u[1] for u in ud]),
                      u_sincos=cand_sincos(np.array([u[2] for u in ud]), np.array([u[3] for u in ud])))
        base, idx, logp = self.step_arrays(inputs, k)
        return base, a_num, idx, logp

    def step_arrays(self, inp, k):
        """One decoder step over N states given as index arrays (see frontier._step_inputs): vp / view [N]
        (feature-table row, view index), a_num [N], cand_view [N,>=A], sincos [N,>=A,4], hrow / crow [N] (pool row
        of h and c, instruction row), has_u [N] and the (u_vp, u_view, u_sincos [N,4]) descriptor of the previous
        action's embedding.  Returns (pool row base of the N new states, top-k action columns [N,k] (-1 = none)
        and their log-probabilities [N,k], numpy); k = 0: the whole row."""
        st, dev = self.store, self.dev
        N = len(inp['vp'])
        A = int(inp['a_num'].max())
        k = min(k, A) if k else A
        # ONE upload: 8 int32 columns of N (each contiguous: no per-column copies on the device), the [N,2] and
        # [N,A] candidate views, then the float32 sin/cos blocks bit-cast into the same int32 buffer
        hu = inp['has_u']
        u_cv_h = np.zeros((N, 2), np.int32)
        u_cv_h[:, 1] = np.where(hu, inp['u_view'], 0)
        u_sc_h = np.zeros((N, 2, 4), np.float32)
        u_sc_h[:, 1] = np.where(hu[:, None], inp['u_sincos'], 0)
        parts = [np.asarray(inp['vp'], np.int32), np.asarray(inp['view'], np.int32), np.asarray(inp['a_num'], np.int32),
                 np.asarray(inp['hrow'], np.int32), np.asarray(inp['crow'], np.int32),
                 np.where(hu, inp['u_vp'], 0).astype(np.int32), hu.astype(np.int32), np.full(N, 2, np.int32),
                 u_cv_h.reshape(-1), np.ascontiguousarray(inp['cand_view'][:, :A], np.int32).reshape(-1),
                 u_sc_h.reshape(-1).view(np.int32),
                 np.ascontiguousarray(inp['sincos'][:, :A], np.float32).reshape(-1).view(np.int32)]
        di = torch.from_numpy(np.concatenate(parts)).to(dev)
        vp, view, a_num, hrow, crow, u_vp, u_act, two = (di[j * N:(j + 1) * N] for j in range(8))
        o = 8 * N
        u_cv = di[o:o + 2 * N].view(N, 2)
        cv = di[o + 2 * N:o + (2 + A) * N].view(N, A)
        o += (2 + A) * N
        u_sc = di[o:o + 8 * N].view(torch.float32).view(N, 2, 4)
        sc = di[o + 8 * N:o + (8 + 4 * A) * N].view(torch.float32).view(N, A, 4)
        df = None
        s = stream()
        new = lambda *sh: torch.empty(*sh, device=dev, dtype=torch.float32)  # noqa: E731
        h0, c0 = new(N, self.H), new(N, self.H)
        H = self.H
        gat = (_lib.RowMove * 2)(_lib.RowMove(self.hpool.buf.data_ptr(), h0.data_ptr(), hrow.data_ptr(), H, H, H, 0),
                                 _lib.RowMove(self.cpool.buf.data_ptr(), c0.data_ptr(), hrow.data_ptr(), H, H, H, 0))
        call('sf_move_rows', gat, 2, N, s)                 # h_t[flat_indices], c_t[flat_indices]: one launch
        ucand = st.cands(u_vp, u_cv, u_sc, two, 2)

        tape = decoder_tape(N, self.H, st.F, self.D, st.V, self.T, A, dev)
        # the previous action's embedding straight into the first half of the LSTM input rows (no copy in the step)
        call('sf_gather_actions_ld', byref(ucand), N, ptr(u_act), ptr(tape['xin']), 2 * st.F, s)
        base, tape['h1'] = self.hpool.reserve(N)
        _, tape['c1'] = self.cpool.reserve(N)
        _, tape['alpha'] = self.apool.reserve(N)
        pano = st.pano(vp, view)
        cnd = st.cands(vp, cv, sc, a_num, A)
        tp = tape_struct(tape)
        with _gate_pass(self):
            call('sf_attn_decoder_fwd', byref(self.w), byref(pano), byref(cnd), N, self.H, self.D, self.T,
                 None, ptr(h0), ptr(c0), ptr(self.ctx), ptr(self.mask), ptr(crow), byref(tp), None,
                 None, 0, *ws_args(dev))
        idx = torch.empty(N, k, dtype=torch.int32, device=dev)
        logp = new(N, k)
        call('sf_logprob_topk', ptr(tape['logit']), A, N, A, ptr(a_num), k, ptr(idx), ptr(logp), s)
        self._keep = (di, df, tape, h0, c0, gat, two, vp, view, a_num, hrow, crow, u_vp, u_act,
                      u_cv, cv, u_sc, sc)
        both = torch.cat((idx.to(torch.float32), logp), dim=1).cpu().numpy()       # ONE D2H copy per iteration
        return base, both[:, :k].astype(np.int64), both[:, k:]

    def step_logprobs(self, inp):
        """`step_arrays` over the whole candidate row: (pool row base, log-probabilities [N, A], -inf where the
        state has no such candidate)."""
        base, order, scores = self.step_arrays(inp, 0)
        logp = np.full(order.shape, -np.inf, np.float32)
        valid = order >= 0
        rows = np.broadcast_to(np.arange(len(order))[:, None], order.shape)
        logp[rows[valid], order[valid]] = scores[valid]
        return base, logp

    def attention_rows(self, rows):
        """Text-attention rows (host) for `attentions` in the result dictionaries."""
        if not rows:
            return []
        r = torch.tensor(rows, dtype=torch.int64, device=self.dev)
        return list(self.apool.buf[r].cpu().numpy())


class GraphStep(_DeviceLoop):
    """The decoder step of the state-factored search as ONE hipGraph over fixed buffers (follower.py:783-836 per
    iteration: observations of the expanded states, `h_t[flat_indices]`, the AttnDecoderLSTM step, log_softmax).

    An iteration expands at most `successor_size` states per instance, so the step has a fixed capacity; what changes
    between iterations is a [8, cap] block of int32 (frontier_core.cpp: fill_inputs) written into pinned memory.  The
    graph: that block H2D; sf_nav_step twice (the states' and their parents' candidate lists straight from the device
    navigation table -- nothing but the eight integers per state is packed on the host); the previous action's
    embedding (sf_gather_actions over the parent's candidates; action 0 = zeros = u_begin); h / c rows from the state
    pool; sf_attn_decoder_fwd with per-state instruction rows; log_softmax in column order; h / c / attention rows of
    the new states scattered to their pool rows; the [cap, A] log-probabilities D2H into pinned memory.  One replay
    and one stream sync per iteration instead of ~25 host-issued launches, an upload and a blocking download.

    Instructions live in a [instances, t_max] buffer (padding masked out), so the graph outlives the minibatch: it is
    captured once per (decoder, store, navigation table, sizes) and re-captured only when a weight (or one of its
    cached layouts) moved or the state pool had to grow."""

    def __init__(self, decoder, store, nav, n_inst, cap, t_max, pool_rows=1 << 14, gate_weights='fp32'):
        self.gate_weights = check_gate_weights(gate_weights)
        dev = store.device
        self.dec, self.store, self.nav, self.dev = decoder, store, nav, dev
        self.n_inst, self.cap, self.T, self.A = n_inst, cap, t_max, nav.A
        self.H = decoder.hidden_size
        self.D = decoder.visual_attention_layer.linear_in_h.weight.shape[0]
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)           # noqa: E731
        i32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int32)             # noqa: E731
        self.pin_in = torch.zeros(8, cap, dtype=torch.int32).pin_memory()
        self.inputs = self.pin_in.numpy()                                            # what fill_inputs writes
        self.dev_in = i32(8, cap)
        A = self.A
        self.obs2, self.obs = _observation_buffers(cap, A, dev)
        self.h0, self.c0 = f32(cap, self.H), f32(cap, self.H)
        self.tape = decoder_tape(cap, self.H, store.F, self.D, store.V, t_max, A, dev)
        self.logp = f32(cap, A)
        self.pin_out = torch.zeros(cap, A, dtype=torch.float32).pin_memory()
        self.out = self.pin_out.numpy()
        self.ctx = f32(n_inst, t_max, self.H)
        self.mask = torch.ones(n_inst, t_max, dtype=torch.uint8, device=dev)
        self.pool_rows = pool_rows
        self.hpool, self.cpool, self.apool = f32(pool_rows, self.H), f32(pool_rows, self.H), f32(pool_rows, t_max)
        self.n = 0
        self.graph = self.baked = None

    # ---- per search
    def load(self, ctx, mask, h, c):
        """The minibatch's encoder outputs: instruction rows 0..B-1, pool rows 0..B-1."""
        B, T = ctx.shape[0], ctx.shape[1]
        if B > self.n_inst or T > self.T:
            raise ValueError('GraphStep built for %d instructions of <= %d tokens' % (self.n_inst, self.T))
        self.mask.fill_(1)
        self.mask[:B, :T].copy_(mask.to(torch.uint8))
        self.ctx[:B, :T].copy_(ctx)
        self.hpool[:B].copy_(h)
        self.cpool[:B].copy_(c)
        self.n = B
        w = _baked_weights(self)                                     # (also refreshes stale cached layouts in place)
        if self.graph is None or w != self.baked:
            self._capture()

    def _issue_steps(self, n_steps):
        for _ in range(n_steps):
            self.dev_in.copy_(self.pin_in, non_blocking=True)
            self._chain()
            self.pin_out.copy_(self.logp, non_blocking=True)

    def _chain(self, n_steps=1, then=None):
        """The launches of a decoder step between the upload of the input block and the download of the
        log-probabilities: `dev_in` -> `logp` over the whole candidate row, the new states' rows scattered to the
        pools, then(stream) if given."""
        # rows 0-1 of the block: nav rows of the states, then of their parents; rows 2-3 their views (fill_inputs)
        d, H = self.dev_in, self.H
        sca = (_lib.RowMove * 3)(*(_lib.RowMove(src.data_ptr(), pool.data_ptr(), d[7].data_ptr(), width, width, width, 1)
                                   for src, pool, width in ((self.tape['h1'], self.hpool, H), (self.tape['c1'], self.cpool, H),
                                                            (self.tape['alpha'], self.apool, self.T))))

        def scatter(s):
            call('sf_move_rows', sca, 3, self.cap, s)
            if then is not None:
                then(s)
        self._keep = (sca, _follower_steps(self, n_steps, self.cap, d[0], d[2], d[4], self.hpool, self.cpool, d[5], d[6],
                                           self.A, None, self.logp, scatter))

    def _capture(self):
        self.pin_in.zero_()
        self.pin_in[7].fill_(-1)                                     # (a warm-up that writes no pool row)
        self.graph = self._capture_steps(1)
        self.baked = _baked_weights(self)

    # ---- the native loop (sim/frontier_core.cpp: run_graph) launches the graph itself
    def native_loop_ready(self):
        return self.graph is not None and hasattr(self.graph, 'raw_cuda_graph_exec') and _hip_entry_points() is not None

    def native_launch_args(self):
        """(hipGraphLaunch, hipStreamSynchronize, graph exec handle, stream handle) as integers."""
        launch, sync = _hip_entry_points()
        return launch, sync, int(self.graph.raw_cuda_graph_exec()), int(torch.cuda.current_stream(self.dev).cuda_stream)

    # ---- per iteration
    def run(self, n):
        """Inputs are in `self.inputs` (columns 0..n-1; the rest padding with destination -1).  Returns the
        log-probabilities [cap, A] (host view, valid until the next run); the new states are pool rows
        self.n - n .. self.n - 1."""
        if self.n + n > self.pool_rows:
            self._grow(self.n + n)
        self.n += n
        self.graph.replay()
        torch.cuda.current_stream().synchronize()
        return self.out

    def _grow(self, need):
        rows = max(2 * self.pool_rows, need)
        for name in ('hpool', 'cpool', 'apool'):
            old = getattr(self, name)
            new = torch.zeros(rows, old.shape[1], device=self.dev, dtype=torch.float32)
            new[:self.n].copy_(old[:self.n])
            setattr(self, name, new)
        self.pool_rows = rows
        keep = self.pin_in.clone()
        self._capture()                                              # the graph holds the pools' addresses
        self.pin_in.copy_(keep)

    def attention_rows(self, rows):
        if not rows:
            return []
        r = torch.tensor(rows, dtype=torch.int64, device=self.dev)
        return list(self.apool[r].cpu().numpy())


_HIP_ENTRY = []


def _hip_entry_points():
    """Addresses of hipGraphLaunch / hipStreamSynchronize in the HIP runtime THIS process has loaded (the one torch and
    libsf_hip.so run on), for the native search loop -- or None."""
    if not _HIP_ENTRY:
        found = None
        try:
            path = None
            with open('/proc/self/maps') as f:
                for line in f:
                    if 'libamdhip64' in line:
                        path = line.split()[-1]
                        break
            if path:
                hip = C.CDLL(path)
                found = (C.cast(hip.hipGraphLaunch, C.c_void_p).value, C.cast(hip.hipStreamSynchronize, C.c_void_p).value)
        except (OSError, AttributeError):
            found = None
        _HIP_ENTRY.append(found)
    return _HIP_ENTRY[0]


def graph_step_key(agent, nav, n_inst, cap, t_max, gate_weights, device_loop=None):
    """device_loop: the sizes of a DeviceStateFactored (its graphs hold other launches than the host loop's step)."""
    key = (id(agent.decoder), id(agent.store), id(nav), n_inst, cap, t_max) + gate_mode_key(gate_weights)
    return key if device_loop is None else key + ('device_loop',) + tuple(device_loop)


def graph_step_for(agent, nav, n_inst, cap):
    """The agent's GraphStep for these sizes (built on first use, kept on the agent)."""
    t_max = agent.max_instruction_length
    # (a captured step keeps the gate-product kernel it was captured with: runtime.strict_gate_product, and the weight
    # storage of Seq2SeqAgent.gate_weights)
    mode = getattr(agent, 'gate_weights', 'fp32')
    key = graph_step_key(agent, nav, n_inst, cap, t_max, mode)
    # (one live configuration: the pools are ~100 MB)
    return _owner_cache(agent, '_graph_steps', key, 1,
                        lambda: GraphStep(agent.decoder, agent.store, nav, n_inst, cap, t_max, gate_weights=mode),
                        dec=agent.decoder, store=agent.store, nav=nav)


class DeviceStateFactored(GraphStep):
    """The state-factored search (follower.py:720-980) with its iteration loop on the device: GraphStep's launch chain
    without the upload of the input block and without the download of the log-probabilities, followed by
    sf_state_factored_select (include/sf_hip.h) -- the bookkeeping of sim/frontier_core.cpp (advance_raw +
    fill_inputs_raw) over tables in device memory, which leaves the next iteration's [8, cap] block in `dev_in`.

    A chunk of `chunk` iterations is ONE replayed hipGraph (graphs = False: issued eagerly); the host reads the status
    words and the per-instance counters once per chunk (`host_reads`) and the used part of the tables once at the end.
    An iteration issued with an empty frontier changes nothing, so every chunk size gives the same tables.  A capacity
    that does not hold a search (node_cap, slot_cap, the state pool) sets an overflow flag: `run` returns None and the
    caller runs the host loop.  The graph is re-captured when a weight (or one of its cached layouts) moved or the pool
    grew, as GraphStep's is.

    Inference only; successor_size * A <= MAX_SUCC, successor_size <= MAX_S, instances <= MAX_B (the lane mapping of the
    kernels) and a decoder with the visual attention."""
    MAX_SUCC, MAX_S, MAX_B = 1024, 64, 256
    NODE_FIELDS = SEARCH_NODE_FIELDS
    SLOT_FIELDS = ('open_key', 'open_node', 'open_pick', 'held_key', 'held_node', 'held_pick')

    def __init__(self, decoder, store, nav, n_inst, completion_size, successor_size, episode_len, key_fields, t_max,
                 chunk=4, graphs=True, node_cap=2048, slot_cap=1024, pool_rows=1 << 14, gate_weights='fp32'):
        if not self.supports(successor_size, n_inst, nav.A, decoder):
            raise ValueError('DeviceStateFactored: %d instances x %d successors x %d candidates is beyond the kernel, or a '
                             'decoder without visual attention' % (n_inst, successor_size, nav.A))
        GraphStep.__init__(self, decoder, store, nav, n_inst, n_inst * successor_size, t_max, pool_rows, gate_weights)
        self.completion, self.successor, self.E, self.key_fields = completion_size, successor_size, episode_len, key_fields
        self.chunk, self.graphs = max(1, int(chunk)), bool(graphs)
        self.node_cap, self.slot_cap, self.visit_cap = int(node_cap), int(slot_cap), int(node_cap)
        # (a visit is a node of its own, so the visits fit whenever the nodes do)
        self.comp_cap = completion_size + successor_size
        per = {4: 36, 3: 12, 2: 1, 1: 0}[key_fields]
        self.n_keys = K = max(nav.scan_rows.values()) * per + 2      # every minibatch's StateSpace.n_keys fits
        B, S = n_inst, successor_size
        segs = [('status', (8,)), ('inst', (B, 8)), ('frontier', (B, S)), ('base_row', (B,)),
                ('comp_order', (B, self.comp_cap)), ('visits', (B, self.visit_cap)),
                ('nodes', (len(self.NODE_FIELDS), B, self.node_cap)), ('slots', (len(self.SLOT_FIELDS), B, self.slot_cap)),
                ('key_tables', (3, B, K))]
        total = sum(int(np.prod(sh)) for _, sh in segs)
        self.state = torch.zeros(total, device=self.dev, dtype=torch.int32)
        self.seg, o = {}, 0
        for name, sh in segs:
            n = int(np.prod(sh))
            self.seg[name] = self.state[o:o + n].view(*sh)
            o += n
        self.o_keys = total - 3 * B * K
        self.n_head = 8 + 8 * B                                      # status + inst: what is read once per chunk
        self.pin_head = torch.zeros(self.n_head, dtype=torch.int32).pin_memory()
        self.last_iterations, self.last_flags = 0, 0
        self.last = None                                    # what the last run returned

    @classmethod
    def supports(cls, successor_size, n_inst=1, A=1, decoder=None):
        return (1 <= successor_size <= cls.MAX_S and successor_size * A <= cls.MAX_SUCC and 1 <= n_inst <= cls.MAX_B
                and (decoder is None or hasattr(decoder, 'visual_attention_layer')))

    def _struct(self):
        g = self.seg
        nodes = {f: g['nodes'][j] for j, f in enumerate(self.NODE_FIELDS)}
        slots = {f: g['slots'][j] for j, f in enumerate(self.SLOT_FIELDS)}
        open_slot, held_slot, comp_node = g['key_tables']
        p = dict(base_row=g['base_row'], status=g['status'], inst=g['inst'], frontier=g['frontier'],
                 open_slot=open_slot, held_slot=held_slot, comp_node=comp_node, comp_order=g['comp_order'],
                 visits=g['visits'], **{'node_' + f: v for f, v in nodes.items()}, **slots)
        return _lib.StateSearch(self.n_inst, self.successor, self.completion, self.E, self.key_fields, self.n_keys,
                                self.node_cap, self.slot_cap, self.visit_cap, self.cap, self.pool_rows, 0,
                                self.nav.struct(), *(p[n].data_ptr() for n in _lib.StateSearch.POINTERS))

    def _issue_steps(self, n_steps):
        ss = self._struct()
        self._chain(n_steps, lambda s: call('sf_state_factored_select', byref(ss), ptr(self.logp), self.A,
                                            ptr(self.dev_in), s))
        self._keep_search = ss

    def _capture(self):
        # an empty frontier for the warm-up and the capture: the selection changes nothing, no pool row is written
        self.state.zero_()
        self.dev_in.zero_()
        self.dev_in[7].fill_(-1)
        self.graph = self._capture_steps(self.chunk, self.graphs)
        self.baked = _baked_weights(self)

    # ---- per search
    def initial_tables(self, space):
        """The search's start as one int32 vector (uploaded in one copy): the roots as node 0 of every instance, in
        "open" with pick -inf, as the first visit and the first frontier; the first input block (fill_inputs_raw).
        Instances beyond the minibatch have their completions from the start: they do nothing."""
        Bn, S, nc = self.n_inst, self.successor, self.node_cap
        B = len(space.items)
        if B > Bn or space.n_keys > self.n_keys:
            raise ValueError('DeviceStateFactored built for %d instances and %d state keys' % (Bn, self.n_keys))
        base = self.n
        sid, key = np.zeros(Bn, np.int64), np.zeros(Bn, np.int64)
        sid[:B], key[:B] = space.root_sid, space.root_key
        root = np.arange(Bn, dtype=np.int64) * nc
        live = np.arange(Bn) < B
        status = np.zeros(8, np.int64)
        status[0], status[1] = B, base
        inst = np.zeros((Bn, 8), np.int64)
        inst[:, 0], inst[:, 1], inst[:, 4], inst[:, 5], inst[:, 6] = 1, 1, 1, live, np.arange(Bn)
        inst[~live, 3] = self.completion
        frontier = np.zeros((Bn, S), np.int64)
        frontier[:, 0] = root
        base_row = np.zeros(Bn, np.int64)
        base_row[:B] = space.base_row
        nodes = np.zeros((len(self.NODE_FIELDS), Bn), np.int64)      # parent sid key action count pool start born score
        nodes[0], nodes[1], nodes[2], nodes[3], nodes[5], nodes[6] = -1, sid, key, -1, np.arange(Bn), 1
        slots = np.zeros((len(self.SLOT_FIELDS), Bn), np.int64)      # open key node pick, held key node pick
        slots[0], slots[1] = key, root
        slots[2] = int(np.array(-np.inf, np.float32).view(np.int32))
        block = np.zeros((8, self.cap), np.int64)
        col = np.where(np.arange(self.cap) < B, np.arange(self.cap), 0)
        s = sid[col]
        block[0], block[1], block[2], block[3] = s // 36, s // 36, s % 36, s % 36
        block[5], block[6] = col, col
        block[7] = np.where(np.arange(self.cap) < B, base + np.arange(self.cap), -1)
        parts = dict(head=np.concatenate((status, inst.reshape(-1), frontier.reshape(-1), base_row)), root=root,
                     nodes=nodes.reshape(-1), slots=slots.reshape(-1), block=block.reshape(-1))
        return parts, np.arange(Bn, dtype=np.int64) * self.n_keys + key

    def _reset(self, space):
        parts, key_at = self.initial_tables(space)
        sizes = [len(v) for v in parts.values()]
        up = torch.from_numpy(np.concatenate(list(parts.values())).astype(np.int32)).to(self.dev)
        head, root, nodes, slots, block = torch.split(up, sizes)
        Bn, g = self.n_inst, self.seg
        self.state[:self.o_keys].zero_()
        self.state[self.o_keys:].fill_(-1)
        self.state[:len(head)].copy_(head)                           # status, inst, frontier, base_row
        g['visits'][:, 0].copy_(root)
        g['nodes'][:, :, 0].copy_(nodes.view(-1, Bn))
        g['slots'][:, :, 0].copy_(slots.view(-1, Bn))
        g['key_tables'][0].view(-1).index_fill_(0, torch.from_numpy(key_at).to(self.dev), 0)     # the roots' open slot
        self.dev_in.copy_(block.view(8, self.cap))

    def run(self, space):
        """One search from the loaded encoder outputs (GraphStep.load) over the minibatch `space`.  Returns the tables
        frontier.hypotheses_from_search_tables reads (host arrays), or None after an overflow flag (`last_flags`)."""
        t0 = time.perf_counter()
        B = len(space.items)
        self._reset(space)
        reads = 0
        while True:
            self._step_chunk(self.graph)
            self.pin_head.copy_(self.state[:self.n_head], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            reads += 1
            n, base, iters, flags = (int(x) for x in self.pin_head[:4])
            if n == 0 or flags:
                break
        self.last_iterations, self.last_flags = iters, flags
        tab = None
        if not flags:
            inst = self.pin_head[8:].view(self.n_inst, 8).numpy().copy()
            n_nodes, n_vis = max(int(inst[:B, 0].max()), 1), max(int(inst[:B, 4].max()), 1)
            g = self.seg
            comp = g['key_tables'][2].gather(1, g['comp_order'].clamp(0, self.n_keys - 1).to(torch.int64))
            flat = torch.cat((g['nodes'][:, :B, :n_nodes].reshape(-1), comp[:B].reshape(-1),
                              g['visits'][:B, :n_vis].reshape(-1))).cpu().numpy()      # the one download of the tables
            reads += 1
            nf = len(self.NODE_FIELDS)
            o1 = nf * B * n_nodes
            o2 = o1 + B * self.comp_cap
            nodes = flat[:o1].reshape(nf, B, n_nodes)
            tab = dict(node_cap=self.node_cap, inst=inst, comp=flat[o1:o2].reshape(B, self.comp_cap),
                       visits=flat[o2:].reshape(B, n_vis), **{f: nodes[j] for j, f in enumerate(self.NODE_FIELDS)})
            tab['score'] = nodes[nf - 1].view(np.float32)
            self.n = base
        self._count_run(reads, t0)
        self.last = tab
        return tab


def device_search_for(agent, nav, n_inst, completion_size, successor_size, key_fields, chunk=None, graphs=None):
    """The agent's DeviceStateFactored for these sizes (buffers and captured graph; built on first use, kept on the
    agent beside -- not among -- the host loop's graph_step_for steps)."""
    t_max = agent.max_instruction_length
    mode = getattr(agent, 'gate_weights', 'fp32')
    chunk = agent.search_chunk if chunk is None else chunk
    graphs = getattr(agent, 'search_graphs', True) if graphs is None else graphs
    sizes = (completion_size, successor_size, agent.episode_len, key_fields, int(chunk), bool(graphs),
             int(agent.search_node_cap), int(agent.search_slot_cap))
    key = graph_step_key(agent, nav, n_inst, n_inst * successor_size, t_max, mode, device_loop=sizes)
    # (one live configuration: the pools are ~100 MB)
    return _owner_cache(agent, '_device_searches', key, 1,
                        lambda: DeviceStateFactored(agent.decoder, agent.store, nav, n_inst, completion_size,
                                                    successor_size, agent.episode_len, key_fields, t_max, chunk, graphs,
                                                    node_cap=agent.search_node_cap, slot_cap=agent.search_slot_cap,
                                                    gate_weights=mode),
                        dec=agent.decoder, store=agent.store, nav=nav)


@gc_paused
def state_factored_search_device(agent, completion_size, successor_size, load_next_minibatch=True, mask_undo=False,
                                 first_n_ws_key=4):
    """Seq2SeqAgent.state_factored_search (follower.py:720-980) through DeviceStateFactored: what
    frontier.state_factored_search returns, assembled by the same code (frontier.state_factored_outputs) from the
    hypothesis table rebuilt out of the device tables.  Returns None when a capacity overflowed (the minibatch is
    loaded; the caller runs the host loop over it).  `agent.device_search` is the DeviceStateFactored used last.
    mask_undo is accepted and ignored, as in the host loop."""
    from . import frontier, nav
    env = agent.env
    _require_store(agent)
    env.reset(sort=True, beamed=True, load_next_minibatch=load_next_minibatch)
    assert env.beam_size >= successor_size
    items = list(env.batch)
    table = nav.table_for(env, agent.store)
    space = frontier.StateSpace(env, table, items, first_n_ws_key)
    ctx, seq_mask, h_t, c_t = _encode_items(agent, items)
    n_inst = getattr(env, 'batch_size', None) or len(items)
    with torch.no_grad():
        ds = device_search_for(agent, table, n_inst, completion_size, successor_size, first_n_ws_key)
        agent.device_search = ds
        ds.load(ctx, seq_mask, h_t, c_t)
        tab = ds.run(space)
        if tab is None:
            if ds.last_flags & _lib.SEARCH_OVF_POOL:                 # the next minibatch finds a larger pool
                ds._grow(2 * ds.pool_rows)
            return None
    t, completed, visits = frontier.hypotheses_from_search_tables(tab, len(items), completion_size)
    return frontier.state_factored_outputs(agent, ds, t, space, completed, visits)


def _search_shape(agent):
    """(instances per minibatch, widest candidate list) of the agent's searches, for DeviceStateFactored.supports."""
    from . import nav
    env = agent.env
    return getattr(env, 'batch_size', None) or len(env.batch), nav.table_for(env, agent.store).A


def device_search_applies(agent, successor_size):
    """Whether state_factored_search runs the device loop for this agent (Seq2SeqAgent.search_on_device is on): the
    native backend, no tie_log, a decoder with the visual attention, a shape the kernel takes."""
    if getattr(agent, 'search_backend', 'native') == 'numpy' or getattr(agent, 'tie_log', None) is not None:
        return False
    if not hasattr(agent.decoder, 'visual_attention_layer') or getattr(agent, 'store', None) is None:
        return False
    n_inst, A = _search_shape(agent)
    return DeviceStateFactored.supports(successor_size, n_inst, A, agent.decoder)


def _require_store(agent):
    if getattr(agent, 'store', None) is None:
        raise RuntimeError('search runs on index-form observations: give the agent a '
                           'features.FeatureStore (agent.store)')
    if not hasattr(agent.env, 'panorama'):
        raise RuntimeError('search needs an env.R2RIndexEnv (index-form observations over the feature table)')


def _encode_items(agent, items):
    """Encoder pass over the minibatch's instructions: (ctx, mask, h_0, c_0), detached."""
    seq, seq_mask, seq_lengths = batch_instructions_from_encoded(
        [it['instr_encoding'] for it in items], agent.max_instruction_length, reverse=agent.reverse_instruction,
        device=agent._device())
    with torch.no_grad():
        ctx, h_t, c_t = agent.encoder(seq, seq_lengths)
    return ctx.detach(), seq_mask, h_t.detach(), c_t.detach()


class FlatSpeakerDecoder:
    """One SpeakerDecoderLSTM step (model.py:487-519) over a flat list of word hypotheses.  pad_rows (default off):
    every step runs over at least that many rows, the hypotheses first, then padding rows (zero state, path 0) whose
    results are dropped -- the row count of the device word loop (DeviceSpeakerBeam), for bit-exact comparisons."""

    def __init__(self, decoder, ctx, path_mask, pad_rows=None):
        from .model import _SPK_TAPE
        self.dec, self.keys = decoder, _SPK_TAPE
        self.ctx = ctx.contiguous()
        self.mask = path_mask.to(torch.uint8).contiguous()
        self.dev = ctx.device
        self.H, self.E = decoder.hidden_size, decoder.embedding.weight.shape[1]
        self.vocab = decoder.decoder2action.weight.shape[0]
        self.ldv = (self.vocab + 3) & ~3
        self.Tp = ctx.shape[1]
        self.hpool, self.cpool, self.apool = _Pool(self.H, self.dev), _Pool(self.H, self.dev), _Pool(self.Tp, self.dev)
        self.w = decoder._w_struct()
        self.pad_rows = pad_rows
        self._keep = None

    def seed(self, h, c):
        B = h.shape[0]
        _, hv = self.hpool.reserve(B)
        _, cv = self.cpool.reserve(B)
        self.apool.reserve(B)
        hv.copy_(h)
        cv.copy_(c)

    def step(self, words, rows, inst, k):
        """words / rows / inst [N]: previous word, pool row of (h, c), path of every hypothesis.  Returns (pool
        row base of the N new states, top-k words [N,k], their log-probabilities [N,k])."""
        dev, H = self.dev, self.H
        n_hyp = len(words)
        k = min(k, self.vocab)
        if self.pad_rows is not None and self.pad_rows > n_hyp:
            pad = self.pad_rows - n_hyp
            words = np.concatenate((np.asarray(words, np.int64), np.full(pad, EOS, np.int64)))
            rows = np.concatenate((np.asarray(rows), np.full(pad, -1)))
            inst = np.concatenate((np.asarray(inst), np.zeros(pad, np.int64)))
        N = len(words)
        ints = torch.from_numpy(np.stack((rows, inst)).astype(np.int32)).to(dev)
        wd = torch.from_numpy(np.asarray(words, np.int64)).to(dev)
        new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
        h0, c0 = new(N, H), new(N, H)
        s_ = stream()
        call('sf_gather_rows', ptr(self.hpool.buf), H, ptr(ints[0]), N, H, ptr(h0), H, s_)
        call('sf_gather_rows', ptr(self.cpool.buf), H, ptr(ints[0]), N, H, ptr(c0), H, s_)
        tape = dict(emb=new(N, self.E), gates=new(N, 4 * H), cat2=new(N, 2 * H), t_text=new(N, H),
                    h_tilde=new(N, H), logit=new(N, self.ldv))
        base, tape['h1'] = self.hpool.reserve(N)
        _, tape['c1'] = self.cpool.reserve(N)
        _, tape['alpha'] = self.apool.reserve(N)
        tp = _lib.SpkDecoderTape(*(tape[key].data_ptr() for key in self.keys))
        call('sf_speaker_decoder_fwd', byref(self.w), N, self.E, H, self.Tp, self.vocab, ptr(wd), ptr(h0), ptr(c0),
             ptr(self.ctx), ptr(self.mask), ptr(ints[1]), byref(tp), None, 0, *ws_args(dev))
        idx = torch.empty(N, k, dtype=torch.int32, device=dev)
        logp = new(N, k)
        call('sf_logprob_topk', ptr(tape['logit']), self.ldv, N, self.vocab, None, k, ptr(idx), ptr(logp), s_)
        self._keep = (ints, wd, h0, c0, tape)
        both = torch.cat((idx.to(torch.float32), logp), dim=1)[:n_hyp].cpu().numpy()
        return base, both[:, :k].astype(np.int64), both[:, k:]

    def attention_rows(self, rows):
        if not rows:
            return []
        return list(self.apool.buf[torch.tensor(rows, dtype=torch.int64, device=self.dev)].cpu().numpy())


class DeviceSpeakerBeam(_DeviceLoop):
    """The speaker's beam search (speaker.py:211-318) with its word loop on the device: R = B * beam_size fixed
    hypothesis slots (instance b owns slots b*beam_size ..), per word step

        h / c of every slot from its parent slot (sf_move_rows), SpeakerDecoderLSTM over all R rows (ctx_row = the
        slot's path; dead rows are decoded and ignored), sf_logprob_topk (k = min(beam_size, vocab)), and
        sf_speaker_beam_select: the next words, parent slots and scores, the completed hypotheses, the history;

    all issued without a host synchronisation.  A chunk of `chunk` word steps is ONE replayed hipGraph (captured once per
    path length Tp on one stream, no forked branches); the host reads the batch's live count once per chunk (4 bytes) and
    the histories once at the end: at most ceil(T / chunk) + 1 reads per minibatch instead of T blocking round trips.
    Steps issued after the search has ended change nothing, so every chunk size gives the same results.  The outputs
    are assembled by the host loop's own code (frontier.speaker_beam_outputs) from the same float32 scores.

    Inference only; beam_size <= MAX_BEAM (one wavefront per instance in the selection kernel)."""
    MAX_BEAM = 64

    def __init__(self, decoder, B, beam_size, T, chunk=8, graphs=True):
        if not self.supports(beam_size):
            raise ValueError('DeviceSpeakerBeam: beam_size %d > %d' % (beam_size, self.MAX_BEAM))
        self.dec, self.dev = decoder, next(decoder.parameters()).device
        self.B, self.beam, self.T = B, beam_size, T
        self.chunk, self.graphs = max(1, int(chunk)), bool(graphs)
        self.H, self.E = decoder.hidden_size, decoder.embedding.weight.shape[1]
        self.vocab = decoder.decoder2action.weight.shape[0]
        self.ldv = (self.vocab + 3) & ~3
        self.k = min(beam_size, self.vocab)
        R = self.R = B * beam_size
        dev = self.dev
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)          # noqa: E731
        self.h0, self.c0 = f32(R, self.H), f32(R, self.H)
        from .model import _SPK_TAPE
        self.keys = _SPK_TAPE
        self.tape = dict(emb=f32(R, self.E), gates=f32(R, 4 * self.H), c1=f32(R, self.H), h1=f32(R, self.H),
                         cat2=f32(R, 2 * self.H), t_text=f32(R, self.H), h_tilde=f32(R, self.H), logit=f32(R, self.ldv))
        self.idx = torch.zeros(R, self.k, device=dev, dtype=torch.int32)
        self.logp = f32(R, self.k)
        self.score = f32(R)
        self.words = torch.full((R,), EOS, device=dev, dtype=torch.int64)
        self.parent = torch.full((R,), -1, device=dev, dtype=torch.int32)
        self.ctx_row = torch.arange(R, device=dev, dtype=torch.int32) // beam_size
        self.head0 = torch.from_numpy(self._record(0).head0()).to(dev)
        self.words0 = self.words.clone()
        self.words0[::beam_size] = BOS
        self.parent0 = self.parent.clone()
        self.parent0[::beam_size] = torch.arange(0, R, beam_size, device=dev, dtype=torch.int32)
        self.Tp = self.Tp_cap = 0                           # the path length of the run at hand, the widest so far
        self.graph_by_tp = {}
        self.baked = None

    @classmethod
    def supports(cls, beam_size):
        return 1 <= beam_size <= cls.MAX_BEAM

    def _record(self, Tp):
        """The record's layout at path length Tp (the header does not depend on it): one download at the end."""
        return BeamRecord(self.B, self.beam, self.T, ('hist_word', 'hist_parent', 'hist_score'), Tp)

    # ---- buffers that depend on the path length (grown, never shrunk: the graphs hold their addresses)
    def _reserve(self, Tp):
        if Tp <= self.Tp_cap:
            return
        dev, B, R = self.dev, self.B, self.R
        self.Tp_cap = Tp
        self.ctx_buf = torch.zeros(B * Tp * self.H, device=dev, dtype=torch.float32)
        self.mask_buf = torch.ones(B * Tp, device=dev, dtype=torch.uint8)
        self.alpha_buf = torch.zeros(R * Tp, device=dev, dtype=torch.float32)
        self.rec = torch.zeros(self._record(Tp).size, device=dev, dtype=torch.int32)
        self.graph_by_tp = {}

    def _views(self, Tp):
        B, R, H = self.B, self.R, self.H
        ctx = self.ctx_buf[:B * Tp * H].view(B, Tp, H)
        mask = self.mask_buf[:B * Tp].view(B, Tp)
        alpha = self.alpha_buf[:R * Tp].view(R, Tp)
        return ctx, mask, alpha

    def _issue_steps(self, n_steps):
        s, Tp, H = stream(), self.Tp, self.H
        ctx, mask, alpha = self._views(Tp)
        rec = self._record(Tp)
        assert self.rec.numel() >= rec.size
        sb = _lib.SpkBeam(self.B, self.beam, self.k, self.T, Tp, EOS, self.score.data_ptr(), self.words.data_ptr(),
                          self.parent.data_ptr(), *rec.pointers(self.rec.data_ptr()))
        tape = dict(self.tape, alpha=alpha)
        tp = _lib.SpkDecoderTape(*(tape[key].data_ptr() for key in self.keys))
        gat = (_lib.RowMove * 2)(_lib.RowMove(tape['h1'].data_ptr(), self.h0.data_ptr(), self.parent.data_ptr(), H, H, H, 0),
                                 _lib.RowMove(tape['c1'].data_ptr(), self.c0.data_ptr(), self.parent.data_ptr(), H, H, H, 0))
        w = self.w
        for _ in range(n_steps):
            call('sf_move_rows', gat, 2, self.R, s)
            call('sf_speaker_decoder_fwd', byref(w), self.R, self.E, H, Tp, self.vocab, ptr(self.words),
                 ptr(self.h0), ptr(self.c0), ptr(ctx), ptr(mask), ptr(self.ctx_row), byref(tp), None, 0,
                 *ws_args(self.dev))
            call('sf_logprob_topk', ptr(self.tape['logit']), self.ldv, self.R, self.vocab, None, self.k, ptr(self.idx),
                 ptr(self.logp), s)
            call('sf_speaker_beam_select', byref(sb), ptr(self.idx), ptr(self.logp), ptr(alpha), s)
        self._keep = (sb, tp, gat, w)

    def _capture(self):
        # dead slots for the warm-up step (every instance ended: the selection changes nothing)
        self.rec[:len(self.head0)].zero_()
        self.words.fill_(EOS)
        self.parent.fill_(-1)
        graph = self.graph_by_tp[self.Tp] = self._capture_steps(self.chunk)
        return graph

    # ---- per minibatch
    def run(self, ctx, path_mask, h, c):
        """One search over the encoder outputs (ctx [B,Tp,H], path_mask [B,Tp], h / c [B,H]).  Returns the host
        arrays (inst [B,3], done_rec / done_score [B, 2 beam], hist_word / hist_parent / hist_score [t_end, R],
        hist_attn [t_end, R, Tp])."""
        t0 = time.perf_counter()
        B, Tp = self.B, ctx.shape[1]
        if ctx.shape[0] != B:
            raise ValueError('DeviceSpeakerBeam built for %d paths, got %d' % (B, ctx.shape[0]))
        self._reserve(Tp)
        self.Tp = Tp
        self.w = self.dec._w_struct()
        wb = bytes(self.w)
        if wb != self.baked:                                             # a weight (or its cached table) moved
            self.graph_by_tp, self.baked = {}, wb
        graph = None
        if self.graphs:
            graph = self.graph_by_tp.get(Tp) or self._capture()
        cv, mv, _ = self._views(Tp)
        cv.copy_(ctx)
        mv.copy_(path_mask.to(torch.uint8))
        self.tape['h1'].view(B, self.beam, self.H)[:, 0].copy_(h)
        self.tape['c1'].view(B, self.beam, self.H)[:, 0].copy_(c)
        rec = self._record(Tp)
        self.rec[:rec.hdr].copy_(self.head0)
        self.words.copy_(self.words0)
        self.parent.copy_(self.parent0)
        self.score.zero_()
        steps, reads = self._run_chunks(graph, self.T, self.rec[rec.o_live:])
        flat = self.rec[:rec.hdr + steps * rec.stride].cpu().numpy()     # the one download of the results
        self._count_run(reads + 1, t0)
        return rec.split(flat, attn='hist_attn')


def speaker_beam_nodes(hist, B, beam_size):
    """The device word loop's histories as the host loop's hypothesis nodes (frontier.speaker_beam_outputs): roots
    0..B-1 (BOS, score 0), then node B + t*R + p for history position p of word step t.  Returns (done, P, W, S, rows)
    with rows[node] the row of its attention in hist_attn.reshape(-1, Tp)."""
    hw, hp, hs = hist['hist_word'], hist['hist_parent'], hist['hist_score']
    t_end, R = hw.shape
    t = np.arange(t_end, dtype=np.int64)[:, None]
    hp64 = hp.astype(np.int64)
    parent = np.where(t == 0, hp64 // beam_size, B + (t - 1) * R + hp64)
    P = np.concatenate((np.full(B, -1, np.int64), parent.reshape(-1)))
    W = np.concatenate((np.full(B, BOS, np.int64), hw.reshape(-1).astype(np.int64)))
    S = np.concatenate((np.zeros(B, np.float32), hs.reshape(-1).astype(np.float32)))
    rows = np.concatenate((np.full(B, -1, np.int64), (t * R + hp64).reshape(-1)))
    n_done = hist['inst'][:, 1]
    done = [[B + int(x) for x in hist['done_rec'][b, :n_done[b]]] for b in range(B)]
    return done, P, W, S, rows


@gc_paused
def speaker_beam_search_device(speaker, beam_size, path_obs, path_actions, chunk=None, graphs=None):
    """Seq2SeqSpeaker.beam_search (speaker.py:211-318) through DeviceSpeakerBeam: the same hypotheses in the same order
    with the same scores, words and attentions as frontier.speaker_beam_search.  The DeviceSpeakerBeam (buffers and
    captured graphs) is kept on the speaker per (decoder, batch, beam, words, chunk, graphs); `speaker.device_beam` is the
    one used last (its host_reads / last_host_reads count the host synchronisations)."""
    from . import frontier
    chunk = speaker.beam_chunk if chunk is None else chunk
    graphs = speaker.beam_graphs if graphs is None else graphs
    start_obs, feats, acts, path_mask, _, _, perm = speaker._batch_observations_and_actions(path_obs, path_actions, None)
    B = len(start_obs)
    with torch.no_grad():
        ctx, h_t, c_t = speaker.encoder(acts, feats)
        key = (id(speaker.decoder), B, beam_size, speaker.instruction_len, int(chunk), bool(graphs))
        db = _owner_cache(speaker, '_device_beams', key, 4, lambda: DeviceSpeakerBeam(
            speaker.decoder, B, beam_size, speaker.instruction_len, chunk, graphs), dec=speaker.decoder)
        speaker.device_beam = db
        hist = db.run(ctx.detach().contiguous(), path_mask, h_t.detach(), c_t.detach())
    done, P, W, S, rows = speaker_beam_nodes(hist, B, beam_size)
    att = hist['hist_attn'].reshape(-1, hist['hist_attn'].shape[-1])
    return frontier.speaker_beam_outputs(start_obs, perm, done, P, W, S, rows, beam_size,
                                         lambda r: list(att[r]) if r else [], getattr(speaker.env, 'tokenizer', None))


class DeviceFollowerBeam(_DeviceLoop):
    """The follower's beam search (follower.py:541-718) with its step loop on the device: R = B * beam_size fixed
    hypothesis slots (instance b owns slots b*beam_size ..), per decode step

        sf_nav_step over the slots' and their parents' states (candidate lists straight from the device navigation
        table), the previous action's embedding from the parent's candidates (sf_gather_actions_ld), h / c of every slot
        from its parent slot (sf_move_rows), AttnDecoderLSTM over all R rows (crow = the slot's instance; dead rows are
        decoded and ignored), sf_logprob_topk (k = min(beam_size, A), n_valid = a_num), and sf_follower_beam_select:
        the next states, parent slots and scores, the completed hypotheses, the history;

    all issued on one stream without a host synchronisation.  A chunk of `chunk` steps is ONE replayed hipGraph; the host
    reads the batch's live count once per chunk (4 bytes) and the history once at the end: at most
    ceil(episode_len / chunk) + 1 reads per minibatch.  Steps issued after the search has ended change nothing, so every
    chunk size gives the same history.  Instructions live in a [B, t_max] buffer (padding masked out), so the graph
    outlives the minibatch; it is re-captured when a weight (or one of its cached layouts) moved.

    Inference only; beam_size <= MAX_BEAM (one wavefront per instance in the selection kernel)."""
    MAX_BEAM = 64
    PLANES = ('parent', 'action', 'rank', 'sid', 'psid', 'score')     # the history arrays besides the attention

    def __init__(self, decoder, store, nav, B, beam_size, episode_len, t_max, chunk=2, graphs=True, gate_weights='fp32'):
        self.gate_weights = check_gate_weights(gate_weights)
        if not self.supports(beam_size, decoder):
            raise ValueError('DeviceFollowerBeam: beam_size %d > %d, or a decoder without visual attention'
                             % (beam_size, self.MAX_BEAM))
        dev = store.device
        self.dec, self.store, self.nav, self.dev = decoder, store, nav, dev
        self.B, self.beam, self.E, self.T, self.A = B, beam_size, episode_len, t_max, nav.A
        self.chunk, self.graphs = max(1, int(chunk)), bool(graphs)
        self.H = decoder.hidden_size
        self.D = decoder.visual_attention_layer.linear_in_h.weight.shape[0]
        self.k = min(beam_size, self.A)
        R = self.R = B * beam_size
        A, H, T = self.A, self.H, t_max
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)           # noqa: E731
        i32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int32)             # noqa: E731
        # slot state: (row, view) of the slots [0, R) and of their parents [R, 2R), previous action, parent slot, score
        self.rv = i32(2, 2 * R)
        self.act, self.parent, self.score = i32(R), i32(R), f32(R)
        self.obs2, self.obs = _observation_buffers(R, A, dev)
        self.h0, self.c0 = f32(R, H), f32(R, H)
        self.tape = decoder_tape(R, H, store.F, self.D, store.V, T, A, dev)
        for v in self.tape.values():
            v.zero_()
        self.idx = i32(R, self.k)
        self.logp = f32(R, self.k)
        self.crow = (torch.arange(R, device=dev, dtype=torch.int32) // beam_size).contiguous()
        self.ctx = f32(B, T, H)
        self.mask = torch.ones(B, T, dtype=torch.uint8, device=dev)
        self.record = BeamRecord(B, beam_size, episode_len, self.PLANES, T)        # one download at the end
        self.rec = i32(self.record.size)
        self.pin = torch.zeros(self.rec.numel(), dtype=torch.int32).pin_memory()
        self.head0 = torch.from_numpy(self.record.head0()).to(dev)
        self.parent0 = torch.full((R,), -1, device=dev, dtype=torch.int32)
        self.parent0[::beam_size] = torch.arange(0, R, beam_size, device=dev, dtype=torch.int32)
        self.graph = self.baked = None
        self.last = None                                    # what the last run returned

    @classmethod
    def supports(cls, beam_size, decoder=None):
        return 1 <= beam_size <= cls.MAX_BEAM and (decoder is None or hasattr(decoder, 'visual_attention_layer'))

    def _issue_steps(self, n_steps):
        fb = _lib.FolBeam(self.B, self.beam, self.k, self.E, self.T, 0, self.nav.struct(),
                          self.score.data_ptr(), self.rv[0].data_ptr(), self.rv[1].data_ptr(), self.act.data_ptr(),
                          self.parent.data_ptr(), *self.record.pointers(self.rec.data_ptr()))
        # (h / c of every slot from its parent slot; crow = the slot's instance)
        self._keep = (fb, _follower_steps(
            self, n_steps, self.R, self.rv[0], self.rv[1], self.act, self.tape['h1'], self.tape['c1'], self.parent,
            self.crow, self.k, self.idx, self.logp,
            lambda s: call('sf_follower_beam_select', byref(fb), ptr(self.idx), ptr(self.logp), ptr(self.tape['alpha']), s)))

    def _capture(self):
        # dead slots for the warm-up step (every instance ended: the selection changes nothing)
        self.rec[:self.record.hdr].zero_()
        self.rv.zero_()
        self.act.zero_()
        self.parent.fill_(-1)
        self.graph = self._capture_steps(self.chunk)

    # ---- per minibatch
    def run(self, ctx, mask, h, c, root_sid):
        """One search over the encoder outputs (ctx [B,T',H], mask [B,T'], h / c [B,H]) from the start states root_sid
        [B].  Returns host arrays: inst [B,3], done_rec / done_score [B, 2 beam], parent / action / rank / sid / psid
        / score [t_end, R], attn [t_end, R, T] (views of one pinned buffer: valid until the next run)."""
        t0 = time.perf_counter()
        B, R, W, rec = self.B, self.R, self.beam, self.record
        Tm = ctx.shape[1]
        if ctx.shape[0] != B or Tm > self.T:
            raise ValueError('DeviceFollowerBeam built for %d instructions of <= %d tokens' % (B, self.T))
        wb = _baked_weights(self)                                        # (also refreshes stale cached layouts in place)
        if wb != self.baked:                                             # a weight (or its cached layout) moved
            self.graph, self.baked = None, wb
        if self.graphs and self.graph is None:
            self._capture()
        self.mask.fill_(1)
        self.mask[:, :Tm].copy_(mask.to(torch.uint8))
        self.ctx[:, :Tm].copy_(ctx)
        self.tape['h1'].view(B, W, self.H)[:, 0].copy_(h)
        self.tape['c1'].view(B, W, self.H)[:, 0].copy_(c)
        sid = np.repeat(np.asarray(root_sid, np.int64), W)               # every slot starts on a valid state
        rv0 = np.stack((np.tile(sid // 36, 2), np.tile(sid % 36, 2))).astype(np.int32)
        self.rv.copy_(torch.from_numpy(rv0))
        self.rec[:rec.hdr].copy_(self.head0)
        self.rec[rec.hdr:].zero_()                                       # (nothing of an earlier search in the download)
        self.rec[rec.hdr:].view(self.E, rec.stride)[:, R:2 * R].fill_(-1)     # action: -1 = no selection there
        self.act.zero_()
        self.parent.copy_(self.parent0)
        self.score.zero_()
        steps, reads = self._run_chunks(self.graph, self.E, self.rec[rec.o_live:])
        n = rec.hdr + steps * rec.stride
        self.pin[:n].copy_(self.rec[:n], non_blocking=True)              # the one download of the results
        torch.cuda.current_stream().synchronize()
        self._count_run(reads + 1, t0)
        self.last = rec.split(self.pin.numpy())
        return self.last


def follower_beam_key(agent, nav, B, beam_size, t_max, chunk, graphs, gate_weights):
    return (id(agent.decoder), id(agent.store), id(nav), B, beam_size, agent.episode_len, t_max, int(chunk),
            bool(graphs)) + gate_mode_key(gate_weights)


def follower_beam_for(agent, nav, B, beam_size, chunk, graphs):
    """The agent's DeviceFollowerBeam for these sizes (buffers and captured graph; built on first use, kept on the
    agent the way graph_step_for keeps its step)."""
    t_max = agent.max_instruction_length
    # (a captured step keeps the gate-product kernel it was captured with: runtime.strict_gate_product, and the weight
    # storage of Seq2SeqAgent.gate_weights)
    mode = getattr(agent, 'gate_weights', 'fp32')
    key = follower_beam_key(agent, nav, B, beam_size, t_max, chunk, graphs, mode)
    return _owner_cache(agent, '_device_beams', key, 4,
                        lambda: DeviceFollowerBeam(agent.decoder, agent.store, nav, B, beam_size, agent.episode_len, t_max,
                                                   chunk, graphs, gate_weights=mode),
                        dec=agent.decoder, store=agent.store, nav=nav)


@gc_paused
def beam_search_device(agent, beam_size, load_next_minibatch=True, mask_undo=False, chunk=None, graphs=None):
    """Seq2SeqAgent.beam_search (follower.py:541-718) through DeviceFollowerBeam: what frontier.beam_search returns,
    assembled by the same code (frontier.beam_outputs) from the hypothesis table rebuilt out of the device history.
    `agent.device_beam` is the DeviceFollowerBeam used last (its host_reads / last_host_reads count the host
    synchronisations).  mask_undo is accepted and ignored, as in the host loop."""
    from . import frontier, nav
    chunk = agent.beam_chunk if chunk is None else chunk
    graphs = agent.beam_graphs if graphs is None else graphs
    env = agent.env
    _require_store(agent)
    env.reset(sort=True, beamed=True, load_next_minibatch=load_next_minibatch)
    assert env.beam_size >= beam_size
    items = list(env.batch)
    table = nav.table_for(env, agent.store)
    space = frontier.StateSpace(env, table, items)
    ctx, seq_mask, h_t, c_t = _encode_items(agent, items)
    with torch.no_grad():
        db = follower_beam_for(agent, table, len(items), beam_size, chunk, graphs)
        agent.device_beam = db
        hist = db.run(ctx, seq_mask, h_t, c_t, space.root_sid)
    t, done = frontier.hypotheses_from_history(space, hist, beam_size)
    att = hist['attn'].reshape(-1, hist['attn'].shape[-1])
    return frontier.beam_outputs(frontier.HistoryAttention(att), t, space, done, beam_size, agent.episode_len)


def beam_search(agent, beam_size, load_next_minibatch=True, mask_undo=False):
    """follower.py:541-718.  Returns (trajs, completed, traversed_lists=None).  With `agent.beam_on_device` the step loop
    runs on the device (beam_search_device); a beam or decoder it cannot take runs the host loop and is counted."""
    from . import frontier
    if getattr(agent, 'beam_on_device', False):
        if DeviceFollowerBeam.supports(beam_size, agent.decoder):
            return beam_search_device(agent, beam_size, load_next_minibatch, mask_undo)
        agent.beam_fallbacks += 1
    return frontier.beam_search(agent, beam_size, load_next_minibatch, mask_undo)


def state_factored_search(agent, completion_size, successor_size, load_next_minibatch=True,
                          mask_undo=False, first_n_ws_key=4):
    """follower.py:720-980.  Returns (trajs, completed_list, traversed_lists).  With `agent.search_on_device` the
    iteration loop runs on the device (state_factored_search_device); a search it does not take (the numpy backend, a
    tie_log, a decoder or shape the kernel does not cover) or that overflowed one of its capacities runs the host loop
    from its start and is counted in `agent.search_fallbacks`."""
    from . import frontier
    if getattr(agent, 'search_on_device', False):
        if device_search_applies(agent, successor_size):
            out = state_factored_search_device(agent, completion_size, successor_size, load_next_minibatch, mask_undo,
                                               first_n_ws_key)
            if out is not None:
                return out
            load_next_minibatch = False                              # (the minibatch is loaded: the host loop re-reads it)
        agent.search_fallbacks += 1
    return frontier.state_factored_search(agent, completion_size, successor_size, load_next_minibatch, mask_undo,
                                          first_n_ws_key)


def speaker_beam_search(speaker, beam_size, path_obs, path_actions):
    """speaker.py:211-318."""
    from . import frontier
    return frontier.speaker_beam_search(speaker, beam_size, path_obs, path_actions)


# ------------------------------------------------------------------------------ pragmatic re-ranking
@gc_paused
def rational_mix(candidate_lists_by_instr_id, speaker_weight):
    """rational_follower.py:117-148: standardise follower and speaker scores over ALL candidates,
    pick per instruction the candidate maximising the weighted sum.  Returns (results, index counts)."""
    lists = list(candidate_lists_by_instr_id.values())
    follower_scores = np.array([c['follower_score'] for l in lists for c in l], np.float64)
    speaker_scores = np.array([c['speaker_score'] for l in lists for c in l], np.float64)
    speaker_std, follower_std = np.std(speaker_scores), np.std(follower_scores)
    sw = speaker_weight / speaker_std
    fw = (1 - speaker_weight) / follower_std
    mixed = speaker_scores * sw + follower_scores * fw           # (the reference's float64 expression, element-wise)
    results, index_count = {}, Counter()
    lo = 0
    for instr_id, candidates in candidate_lists_by_instr_id.items():
        best_ix = int(np.argmax(mixed[lo:lo + len(candidates)]))   # first maximum, like max() over enumerate
        lo += len(candidates)
        results[instr_id] = candidates[best_ix]
        index_count[best_ix] += 1
    return results, index_count


# ------------------------------------------------------------------------------ rational speaker
def generate_and_score_candidates(envir, speaker, follower, n_candidates, include_gold=False):
    """rational_speaker.py:9-106: for every gold path of the environment the speaker's `n_candidates` beam
    instructions (speaker.py:211-318), each scored by the follower with teacher forcing along that path
    (follower.py:342-428: how likely is THIS route given that instruction).  Returns {instr_id: [candidate, ...]},
    every candidate with `speaker_score`, `follower_score` and the follower's `actions`; stops when an instruction
    comes round again (one epoch)."""
    from .follower import EOS
    follower.env = envir
    speaker.env = envir
    envir.reset_epoch()
    speaker.feedback = 'argmax'
    for module in (follower.encoder, follower.decoder, speaker.encoder, speaker.decoder):
        module.eval()
    follower.set_beam_size(1)
    by_id = {}
    n_per_instance = []
    looped = False
    while not looped:
        path_obs, path_actions, gold_instr = envir.gold_obs_actions_and_instructions(speaker.max_episode_len,
                                                                                     load_next_minibatch=True)
        with torch.no_grad():
            gold = []
            if include_gold:
                gold, _ = speaker._score_obs_actions_and_instructions(path_obs, path_actions, gold_instr, 'teacher')
            beams = speaker.beam_search(n_candidates, path_obs, path_actions)
            if include_gold:
                assert len(gold) == len(beams)
                for g, bc in zip(gold, beams):
                    assert g['instr_id'] == bc[0]['instr_id']
                    bc.insert(0, g)
            cand_obs, cand_actions, cand_words = [], [], []
            for i, beam in enumerate(beams):
                n_per_instance.append(len(beam))
                for cand in beam:
                    cand_obs.append(path_obs[i])
                    cand_actions.append(path_actions[i])
                    idx = list(cand['word_indices'])
                    cand_words.append(idx[:-1] if idx and idx[-1] == EOS else idx)      # rational_speaker.py:63-65
            scored, _ = follower._score_obs_actions_and_instructions(cand_obs, cand_actions, cand_words)
        assert len(scored) == sum(len(b) for b in beams)
        k = 0
        for beam in beams:
            for cand in beam:
                fs = scored[k]
                k += 1
                assert cand['instr_id'] == fs['instr_id']
                cand['speaker_score'], cand['follower_score'], cand['actions'] = cand['score'], fs['score'], fs['actions']
            instr_id = beam[0]['instr_id']
            assert all(c['instr_id'] == instr_id for c in beam)
            if instr_id in by_id:
                looped = True
            else:
                by_id[instr_id] = beam
    return by_id


def predict_from_candidates(candidate_lists_by_instr_id, speaker_weights):
    """rational_speaker.py:109-137: scores standardised over ALL candidates; per weight and instruction the
    candidate with the highest weighted sum (first maximum).  Returns {weight: {instr_id: candidate}}."""
    return {w: rational_mix(candidate_lists_by_instr_id, w)[0] for w in speaker_weights}


def run_rational_speaker(envir, speaker_evaluator, speaker, follower, n_candidates, include_gold=False):
    """rational_speaker.py:140-165 without the file output: candidates, re-ranking for the 21 speaker weights 0, 0.05 ..
    1, and -- with an evaluator (eval_speaker.py's BLEU scoring: speaker_evaluation.SpeakerEvaluation, or any object
    with score_results) -- its score summary per weight.  Returns
    (scores_by_weight or None, results_by_weight)."""
    by_id = generate_and_score_candidates(envir, speaker, follower, n_candidates, include_gold)
    weights = [float(w) for w in np.arange(0, 20 + 1) / 20.0]
    results = predict_from_candidates(by_id, weights)
    scores = None
    if speaker_evaluator is not None:
        scores = {w: speaker_evaluator.score_results(r)[0] for w, r in results.items()}
    return scores, results


def _follower_candidates(follower, beam_size, include_gold, mask_undo, state_factored, key_fields):
    """One minibatch of candidate routes per instruction (rational_follower.py:35-62): optionally the gold route
    (a teacher-forced rollout) first, then the (state-factored) beam search's completions."""
    gold = []
    if include_gold:
        follower.feedback = 'teacher'
        gold = follower._rollout_with_loss()
    follower.feedback = 'argmax'
    if state_factored:
        cands, hyps, walks = follower.state_factored_search(beam_size, 1, load_next_minibatch=not include_gold,
                                                            mask_undo=mask_undo, first_n_ws_key=key_fields)
    else:
        cands, hyps, walks = follower.beam_search(beam_size, load_next_minibatch=not include_gold, mask_undo=mask_undo)
    if include_gold:
        assert len(gold) == len(cands)
        for g, c in zip(gold, cands):
            assert g['instr_id'] == c[0]['instr_id']
            c.insert(0, g)
    return cands, hyps, walks


def _walked_route(walk_so_far, hyp):
    """What the agent physically walks to END at `hyp` after the search (rational_follower.py:87-96): the
    search's own traversal, then from its last state to the candidate's end state."""
    tail = least_common_viewpoint_path(walk_so_far[-1], hyp)[1:]
    return [path_element_from_observation(s.observation) for s in list(walk_so_far) + tail]


def run_rational_follower(envir, evaluator, follower, speaker, beam_size, include_gold=False,
                          compute_oracle=False, mask_undo=False, state_factored_search=False,
                          state_first_n_ws_key=4, physical_traversal=False,
                          speaker_weights=(0., 0.95)):
    """rational_follower.py:12-190 without the file outputs: follower candidates by (state-factored)
    beam search, every candidate route scored by the speaker with teacher forcing (how likely is THIS
    instruction given that route), candidates re-ranked by `rational_mix` for every speaker weight.
    `evaluator` (eval.py: evaluation.Evaluation of this package) is optional: with one, returns its score
    summaries per weight like the reference; without, the chosen candidates per weight."""
    follower.env = envir
    envir.reset_epoch()
    for module in (follower.encoder, follower.decoder, speaker.encoder, speaker.decoder):
        module.eval()
    follower.set_beam_size(beam_size)
    # the search hands its routes to the speaker in index form the moment its last iteration is done: the device scores
    # them while the host builds their result dictionaries (a gold route in front of every list changes the batch: off)
    follower.candidates_hook = (speaker.route_scores_hook('teacher')
                                if state_factored_search and not include_gold and hasattr(speaker, 'route_scores_hook')
                                else None)
    by_instruction = {}
    while True:                                         # one epoch: until an instruction comes round again
        cands, hyps, walks = _follower_candidates(follower, beam_size, include_gold, mask_undo, state_factored_search,
                                                  state_first_n_ws_key)
        flat = flatten(cands)
        with torch.no_grad():
            spoken, _ = speaker._score_obs_actions_and_instructions(
                [c['observations'] for c in flat], [c['actions'] for c in flat], [c['instr_encoding'] for c in flat],
                feedback='teacher')
        assert len(spoken) == len(flat)
        for c, sp in zip(flat, spoken):
            assert c['instr_id'] == sp['instr_id']
            c['follower_score'], c['speaker_score'] = c['score'], sp['score']
            del c['observations']
        wrapped = False
        if physical_traversal:
            for b, group in enumerate(cands):
                offset = 1 if include_gold else 0       # the gold route is not a search hypothesis
                for c, hyp in zip(group[offset:], hyps[b]):
                    route = _walked_route(walks[b], hyp)
                    assert route[-1][0] == c['trajectory'][-1][0]
                    c['trajectory'] = route
        if compute_oracle and evaluator is not None:
            if hasattr(evaluator, 'score_routes'):      # every candidate of the minibatch in one batch (one launch)
                scored = evaluator.score_routes([c['instr_id'] for c in flat], [c['trajectory'] for c in flat])
            else:
                scored = [evaluator._score_item(c['instr_id'], c['trajectory']) for c in flat]
            for c, r in zip(flat, scored):
                c['eval_result'] = r._asdict()
        for group in cands:
            instr_id = group[0]['instr_id']
            assert all(c['instr_id'] == instr_id for c in group)
            if instr_id in by_instruction:
                wrapped = True
            else:
                by_instruction[instr_id] = group
        if wrapped:
            break
    follower.candidates_hook = None
    outcome, picks = {}, {}
    for w in speaker_weights:
        chosen, picks[w] = rational_mix(by_instruction, w)
        outcome[w] = evaluator.score_results(chosen)[0] if evaluator is not None else chosen
    return outcome, picks
