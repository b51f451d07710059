"""Follower rollout on the HIP path.

* `batch_instructions_from_encoded` -- host-side instruction batching with the reference's
  semantics (follower.py:75-105).
* `DeviceFollowerBatch` / `FollowerEngine` -- the whole follower episode
  (Seq2SeqAgent._rollout_with_loss, follower.py:430-539, and
  _score_obs_actions_and_instructions, :342-428) as a sync-free sequence of C-ABI calls over
  index-form observations: encoder, then per step decoder + glue, with the argmax /
  teacher feedback, `ended` flags, u_prev gather and loss terms all kept on the device.
  Training: `engine.rollout(...).loss.backward()` runs BPTT through the C-ABI backward
  entry points, accumulating weight gradients in place.
"""
import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import call
from .features import cand_sincos
from .model import (decoder_params, decoder_w_struct, _encoder_structs, _TAPE_KEYS,
                    grad_ptr, trainable_embedding, bi_encoder_tapes, bi_encoder_fwd, bi_encoder_bwd)
from .runtime import ptr, stream, ws_args, wgrad_ws_args, ensure_workspace, dropout_arg, fill_regions, fault_bits, reissue_per_step, concurrent_stream, graph_capture, WeightsMoved, transposed, check_gate_weights, gate_weights_pass, register_bf16_weights
from .dp import collectives_on

byref = C.byref

PAD, UNK, EOS, BOS = 0, 1, 2, 3      # utils.py:19-24
FEEDBACK = {'teacher': 0, 'argmax': 1, 'sample': 2}


def batch_instructions_from_encoded(encoded_instructions, max_length, reverse=False, sort=False,
                                    device=None):
    """follower.py:75-105.  Returns (seq [B,max_length] int64, mask [B,max(len)] bool
    (True = PAD), lengths list[, perm list]); tensors on `device` (default: cuda if present)."""
    # (rows that are the SAME object -- the candidate routes of one instruction in the pragmatic re-ranking,
    # rational_follower.py:67-69 -- are encoded once)
    first, src = {}, []
    for inst in encoded_instructions:
        j = first.get(id(inst))
        if j is None:
            j = first[id(inst)] = len(first)
        src.append(j)
    distinct = [None] * len(first)
    for inst, j in zip(encoded_instructions, src):
        distinct[j] = inst
    seq = np.full((len(distinct), max_length), PAD, np.int64)
    lengths = []
    for i, inst in enumerate(distinct):
        inst = np.asarray(inst, np.int64)
        if len(inst) > 0:
            assert inst[-1] != EOS
        if reverse:
            inst = inst[::-1]
        inst = np.concatenate((inst, [EOS]))[:max_length]
        seq[i, :len(inst)] = inst
        lengths.append(len(inst))
    if len(distinct) < len(src):
        seq = seq[src]
        lengths = [lengths[j] for j in src]
    perm = None
    if sort:
        perm = np.argsort(-np.asarray(lengths), kind='stable')
        lengths = [lengths[i] for i in perm]
        seq = seq[perm]
    mask = (seq == PAD)[:, :max(lengths)]
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    seq_t = torch.from_numpy(seq).to(device)
    mask_t = torch.from_numpy(np.ascontiguousarray(mask)).to(device)
    if sort:
        return seq_t, mask_t, lengths, list(perm)
    return seq_t, mask_t, lengths


@dataclass
class DeviceFollowerBatch:
    """Index-form episode batch resident in HBM (see synth.FollowerBatch for the fields)."""
    seq: torch.Tensor          # [B,Lpad] int64
    lengths: list
    lengths_dev: torch.Tensor  # [B] int32
    mask: torch.Tensor         # [B,T] uint8, 1 = PAD
    vp: torch.Tensor           # [S,B] int32
    view: torch.Tensor         # [S,B] int32
    a_num: torch.Tensor        # [S,B] int32
    cand_view: torch.Tensor    # [S,B,A] int32
    sincos: torch.Tensor       # [S,B,A,4] fp32
    target: torch.Tensor       # [S,B] int64
    a_max: int
    row0: int = 0              # global id of row 0 (data-parallel shard offset)

    @property
    def batch_size(self):
        return self.seq.shape[0]

    @classmethod
    def from_synth(cls, fb, device='cuda', max_length=80, reverse=True, rows=None, row0=0):
        """Upload a synth.FollowerBatch (optionally only `rows`, a slice, for data parallelism)."""
        sl = rows if rows is not None else slice(None)
        instr = fb.instr[sl]
        seq, mask, lengths = batch_instructions_from_encoded(instr, max_length, reverse=reverse,
                                                             device=device)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)  # noqa: E731
        return cls(seq=seq, lengths=lengths,
                   lengths_dev=torch.tensor(lengths, dtype=torch.int32, device=device),
                   mask=mask.to(torch.uint8).contiguous(),
                   vp=dev(fb.vp[:, sl], torch.int32), view=dev(fb.view[:, sl], torch.int32),
                   a_num=dev(fb.a_num[:, sl], torch.int32),
                   cand_view=dev(fb.cand_view[:, sl], torch.int32),
                   sincos=dev(cand_sincos(fb.cand_heading[:, sl], fb.cand_elevation[:, sl]),
                              torch.float32),
                   target=dev(fb.target[:, sl], torch.int64), a_max=fb.a_max, row0=row0)


def route_index_batch(path_obs, path_actions, encoded_instructions, episode_len, a_max=None):
    """Given routes (follower.py:342-428's input) -> (synth.FollowerBatch with [S,B] grids, S) for a teacher-forced
    FollowerEngine pass, in the host loop's layout: step t < len(actions) of row b stands at obs[t] with target
    actions[t], later steps repeat the last of those observations with target -1.  S is the step at which the host loop
    stops: every row has taken action 0 (its own stop, or the clamped -1 behind a route that ends without one), at most
    `episode_len`.  Every distinct observation dictionary is read once (the candidate instructions of one route share
    its observations, rational_speaker.py:54-69).  Raises ValueError on what the device pass cannot reproduce: an empty
    route, an action outside the candidates, an action 0 before the last action (the engine latches `ended`,
    csrc/sf_glue.h; the host loop goes on scoring the targets behind it)."""
    from .synth import FollowerBatch
    B = len(path_obs)
    if len(path_actions) != B or len(encoded_instructions) != B:
        raise ValueError('%d routes, %d action lists, %d instructions' % (B, len(path_actions), len(encoded_instructions)))
    stop = np.empty(B, np.int64)                  # the step at which row b takes action 0
    for b, (obs, acts) in enumerate(zip(path_obs, path_actions)):
        m = len(acts)
        if m == 0 or len(obs) < m:
            raise ValueError('route %d: %d actions over %d observations' % (b, m, len(obs)))
        z = next((t for t, a in enumerate(acts) if a == 0), m)
        if z < m - 1 and z < episode_len - 1:
            raise ValueError('route %d stops at step %d of %d: the device pass scores no target behind a stop' % (b, z, m))
        stop[b] = z
    S = int(min(episode_len, stop.max() + 1))
    slot, distinct = {}, []
    at = np.empty((S, B), np.int64)               # [S,B] -> index into `distinct`
    target = np.full((S, B), -1, np.int64)
    for b, (obs, acts) in enumerate(zip(path_obs, path_actions)):
        m = len(acts)
        for t in range(S):
            ob = obs[min(t, m - 1)]
            k = slot.get(id(ob))
            if k is None:
                k = slot[id(ob)] = len(distinct)
                distinct.append(ob)
            at[t, b] = k
            if t < m:
                target[t, b] = acts[t]
    adj = [ob['adj_loc_list'] for ob in distinct]
    n_adj = np.array([len(x) for x in adj], np.int32)
    A = int(a_max or n_adj.max())
    D = len(distinct)
    d_vp, d_view = np.empty(D, np.int32), np.empty(D, np.int32)
    d_cv = np.zeros((D, A), np.int32)
    d_h, d_e = np.zeros((D, A), np.float64), np.zeros((D, A), np.float64)      # (sin / cos taken in float64, env.py:69-74)
    for k, (ob, cands) in enumerate(zip(distinct, adj)):
        d_vp[k], d_view[k] = ob['vp_row'], ob['viewIndex']
        for a, d in enumerate(cands[1:], 1):
            d_cv[k, a], d_h[k, a], d_e[k, a] = d['absViewIndex'], d['rel_heading'], d['rel_elevation']
    a_num = n_adj[at]
    bad = (target != -1) & ((target < 0) | (target >= a_num))
    if bad.any():
        t, b = np.argwhere(bad)[0]
        raise ValueError('route %d, step %d: action %d of %d candidates' % (b, t, target[t, b], a_num[t, b]))
    fb = FollowerBatch(instr=list(encoded_instructions), vp=d_vp[at], view=d_view[at], a_num=a_num,
                       cand_view=d_cv[at], cand_heading=d_h[at], cand_elevation=d_e[at], target=target, a_max=A)
    return fb, S


def scored_route_outputs(path_obs, path_actions, actions, step_scores, live):
    """follower.py:342-428's result dictionaries from a teacher-forced pass over route_index_batch's grids: actions,
    step_scores, live [S,B] as the engine leaves them.  The host loop's bookkeeping: a row records steps up to and
    including the first at which it takes action 0; 'trajectory' is the first observation, then the observation of
    every recorded step (so the first one twice, and the repeated last one behind a route that ends without a stop);
    'scores' are the step scores of live targets (0 for the clamped -1), 'score' their float32 running sum in step
    order; 'observations' holds the first observation only."""
    acts = np.asarray(actions).astype(np.int64)
    sc = np.asarray(step_scores, np.float32) * np.asarray(live, np.float32)       # (score * live, :405)
    S = acts.shape[0]
    ss = np.add.accumulate(sc, axis=0, dtype=np.float32)                          # (sequential float32 sums)
    is0 = acts == 0
    last = np.where(is0.any(0), is0.argmax(0), S - 1).tolist()
    acts_l, sc_l, ss_l = acts.T.tolist(), sc.T.tolist(), ss.T.tolist()
    out = []
    for b, (obs, pa) in enumerate(zip(path_obs, path_actions)):
        k, m = last[b] + 1, len(pa)
        o0 = obs[0]
        steps = [o0] + [obs[t] for t in range(min(k, m))] + [obs[m - 1]] * max(0, k - m)
        out.append({'instr_id': o0['instr_id'],
                    'trajectory': [(ob['viewpoint'], ob['heading'], ob['elevation']) for ob in steps],
                    'actions': acts_l[b][:k], 'scores': sc_l[b][:k], 'observations': [o0],
                    'instr_encoding': o0['instr_encoding'], 'score': ss_l[b][k - 1]})
    return out


class RolloutState:
    """Everything one rollout keeps in HBM: per-step tapes and the glue outputs."""
    pass


class _RolloutLossFn(torch.autograd.Function):
    """Connects the engine's device-side loss to torch autograd: backward() runs BPTT."""

    @staticmethod
    def forward(ctx, engine, state, *params):
        ctx.engine, ctx.state = engine, state
        return state.loss_buf.clone().reshape(())

    @staticmethod
    def backward(ctx, dloss):
        if ctx.state is None:
            raise RuntimeError('second backward through a pass whose tape the first backward released')
        ctx.engine._backward(ctx.state, dloss)
        # state -> loss -> grad_fn -> ctx -> state is a reference cycle: a few hundred MB of tape per pass that only
        # the cyclic collector would free (seen as a 4 GB sawtooth under a training loop).  The tape has been consumed.
        ctx.state = None
        return (None, None) + (None,) * (len(ctx.needs_input_grad) - 2)


PROJECT_MAX_B = 256         # largest batch of the projected decode chain (the split attention's limit, csrc/sf_kernels.h)


class projected_pass:
    """`with projected_pass(on):` -- whether the decode steps issued inside look the projected tables up
    (sf_projected_use; process-wide like the gate product's switches).  Restores the switch on exit."""

    def __init__(self, on):
        self.on = int(bool(on))

    def __enter__(self):
        self.prev = int(_lib.lib.sf_projected_is_used())
        if self.prev != self.on:
            _lib.lib.sf_projected_use(self.on)
        return self

    def __exit__(self, *exc):
        if self.prev != self.on:
            _lib.lib.sf_projected_use(self.prev)
        return False


class gate_rows_pass:
    """`with gate_rows_pass(on):` -- whether the projected decode steps issued inside look the gate-space rows up
    (sf_gate_rows_use; process-wide like projected_pass).  Restores the switch on exit."""

    def __init__(self, on):
        self.on = int(bool(on))

    def __enter__(self):
        self.prev = int(_lib.lib.sf_gate_rows_is_used())
        if self.prev != self.on:
            _lib.lib.sf_gate_rows_use(self.on)
        return self

    def __exit__(self, *exc):
        if self.prev != self.on:
            _lib.lib.sf_gate_rows_use(self.prev)
        return False


class gate_rows_attended_pass:
    """`with gate_rows_attended_pass(on):` -- whether the steps that run on gate-space rows also look the attended half's
    table up (sf_gate_rows_attended_use; process-wide like gate_rows_pass).  Restores the switch on exit."""

    def __init__(self, on):
        self.on = int(bool(on))

    def __enter__(self):
        self.prev = int(_lib.lib.sf_gate_rows_attended_is_used())
        if self.prev != self.on:
            _lib.lib.sf_gate_rows_attended_use(self.on)
        return self

    def __exit__(self, *exc):
        if self.prev != self.on:
            _lib.lib.sf_gate_rows_attended_use(self.prev)
        return False


class gate_rows_recurrent_pass:
    """`with gate_rows_recurrent_pass(on):` -- whether the steps that run on both gate-space rows also take the recurrent
    half of their gates as a row launch (2) of the step before formed (sf_gate_rows_recurrent_use; process-wide like
    gate_rows_attended_pass).  Restores the switch on exit."""

    def __init__(self, on):
        self.on = int(bool(on))

    def __enter__(self):
        self.prev = int(_lib.lib.sf_gate_rows_recurrent_is_used())
        if self.prev != self.on:
            _lib.lib.sf_gate_rows_recurrent_use(self.on)
        return self

    def __exit__(self, *exc):
        if self.prev != self.on:
            _lib.lib.sf_gate_rows_recurrent_use(self.prev)
        return False


class FollowerEngine:
    def __init__(self, encoder, decoder, store, group=None):
        self.encoder, self.decoder, self.store = encoder, decoder, store
        self.group = group              # torch.distributed process group for data parallelism
        self.iteration = 0              # rollouts issued so far
        self.site_next = 0              # first unused dropout / sampling site (see rollout)
        # device-side site counter (capture_training): when set, the kernels receive stream ids RELATIVE to this word
        # and `site_next` only mirrors it on the host
        self.site_word = None
        self.dropout_seed = None
        self.two_stream_backward = True  # heads of the backward on a side stream (see sf_follower_episode_bwd)
        self._side_stream = None
        self.grad_sync = None            # dp.BucketedGrads(dp.follower_buckets(enc, dec)): all-reduce launched from the backward
        self._open_forks = []            # side streams forked from the current one and not joined yet (_backward)
        self.fold_text = True            # inference rollouts: text attention over ctx W_in / ctx W_out[:, :H]^T (ABI 9)
        self.pipelined = True           # head(t+1) next to tail(t) in paired launches (sf_hip.h)
        self.episode_call = True        # the whole decode loop (and its backward) as ONE C call
        self.fused_env_step = True      # nav.DeviceNavBatch: the env step inside the scoring + glue launch
        self.fallbacks = 0              # rollouts re-issued on the per-step kernels after a persistent-launch fault (run)
        self._gate_weights = 'fp32'
        self._project = 'auto'
        self.gate_rows = True           # projected rollouts: the action half of the LSTM input as a gate-space row (below)
        # ... and the image part of the attended half too (sf_gate_rows_attended_build): the product shrinks to K = LOC + H.
        # Means something only while `gate_rows` is on; built, used and refreshed with those rows
        self.gate_rows_attended = True
        # ... and the recurrent half of the next step's gates (h1 W_hh^T + biases) as product blocks of launch (2)
        # (sf_gate_rows_recurrent_use): the cell behind is a product over K = LOC that adds three rows.  Means something only
        # while `gate_rows_attended` is on; needs no table
        self.gate_rows_recurrent = True
        self._capturing = False         # inside capture() / capture_sharded(): 'auto' builds the projected tables

    # The two-chain forward schedule (the visual half of step t + 1 on a side stream) is retired: DESIGN.md section 9.
    # The name stays because callers still assign it; asking for the schedule fails instead of measuring the default.
    @property
    def two_stream_forward(self):
        return False

    @two_stream_forward.setter
    def two_stream_forward(self, on):
        if on:
            raise ValueError('two_stream_forward is retired (DESIGN.md section 9): the forward runs on one stream')

    # Whether inference rollouts score and attend on the PROJECTED feature tables of (store, decoder) -- two dependent
    # launches per decode step behind the cell instead of four (include/sf_hip.h: sf_projected_build;
    # features.FeatureStore.projected).  The tables cost 1.57 GB for the full R2R table and about 13 ms to build, so:
    #   'auto' (default)  capture() / capture_sharded() build them (a captured rollout is replayed many times); an eager
    #                     rollout() USES tables that exist already for its (store, decoder) -- it then launches the kernels
    #                     a replay does -- but never builds them.  One exception keeps "a replay equals the eager rollout"
    #                     true in both orders: once a pair has run an inference rollout unprojected, a later capture()
    #                     leaves it unprojected too (FeatureStore.note_unprojected) -- for the life of the pair, and only
    #                     `state.projected` shows it.  Capture first, or set True, to get the two-launch chain
    #   True              built on first use, by an eager rollout too
    #   False             never used
    # Only a rollout that takes the folded text stage can be projected (inference, index-form fp32 store, B <= 256, not a
    # device-resident environment); every other one runs the chain it always ran.  `state.projected` says which ran.
    # The switch reaches the library as a PROCESS-WIDE flag set around the episode call (projected_pass), and
    # `state.projected` is read off a process-wide step counter: engines that issue rollouts concurrently from several host
    # threads must agree on `project` (the library's other switches -- gate_weights_pass -- have the same limit).
    @property
    def project(self):
        return self._project

    @project.setter
    def project(self, mode):
        if not (mode is True or mode is False or mode == 'auto'):
            raise ValueError("project must be 'auto', True or False, not %r" % (mode,))
        self._project = mode

    def _projected_tables(self, B, build=None, T=1, A=1):
        """The (store, decoder) tables this engine's policy lets a rollout of batch B (context width T, A candidate slots)
        use now, or None.  Nothing is built -- and the pair is not marked -- for a shape or a store the chain declines."""
        store = self.store
        if self._project is False or B > PROJECT_MAX_B or store.dtype != 'fp32':
            return None
        if not _lib.lib.sf_projected_supported(B, self.decoder.hidden_size, T, A, store.V, store.IMG, store.LOC):
            return None
        if build is None:
            # 'auto' builds inside capture() -- unless this (store, decoder) has already handed out unprojected inference
            # results in this process: the replay then stays, bit for bit, the eager rollout made before the capture
            build = self._project is True or (self._capturing and not self.store.seen_unprojected(self.decoder))
        hit = self.store.projected(self.decoder, build=build)
        if hit is None and self._project == 'auto' and not self._capturing:
            self.store.note_unprojected(self.decoder)
        return hit

    def _gate_rows_tables(self, projected, train):
        """The gate-space rows (include/sf_hip.h: sf_gate_rows_build; FeatureStore.gate_rows) a rollout that runs on the
        projected tables `projected` may use now, or None.  They ride on the projected chain and follow its policy: built
        where that policy builds (`project = True`, or 'auto' inside capture()), otherwise used only if they exist.  Never
        with `gate_weights = 'bf16'` (the packed images cover the whole W_ih) and never with `gate_rows = False`: such
        rollouts launch the gate product over the whole input, bit for bit what they did without the tables."""
        if projected is None or not self.gate_rows or self.pass_gate_weights(train) != 'fp32':
            return None
        # (the store's default keeps the attended half's table beside them; only `gate_rows_attended = False` says otherwise)
        opt = {} if self.gate_rows_attended else {'attended': False}
        return self.store.gate_rows(self.decoder, build=self._project is True or self._capturing, **opt)

    # How the decoder LSTM's weights are stored for the gate product of INFERENCE passes: 'fp32' (default) or 'bf16'
    # (include/sf_hip.h: sf_gate_product_bf16_weights -- the product of the unrounded activations with the weights rounded
    # to bf16 once; half the bytes per decode step).  A pass that keeps a tape for a backward (train mode, or parameters that
    # require grad under grad mode) ignores it: a forward on rounded weights against a backward on unrounded ones would be
    # wrong.  A captured rollout keeps the mode it was captured with.
    @property
    def gate_weights(self):
        return self._gate_weights

    @gate_weights.setter
    def gate_weights(self, mode):
        self._gate_weights = check_gate_weights(mode)

    def pass_gate_weights(self, train=None):
        """The weight storage a rollout issued NOW with `train` runs its gate products on."""
        if self._gate_weights == 'fp32':
            return 'fp32'
        enc, dec = self.encoder, self.decoder
        taped = (dec.training if train is None else train) or (torch.is_grad_enabled() and any(
            p.requires_grad for p in list(enc.parameters()) + list(dec.parameters())))
        return 'fp32' if taped else self._gate_weights

    # ------------------------------------------------------------------------------ forward
    def rollout(self, batch, steps, feedback='argmax', train=None, finalize=True):
        """Runs encoder + `steps` decode steps.  Returns a RolloutState with
        .logits [S,B,A] (masked), .actions [S,B], .step_scores [S,B], .loss (0-dim tensor,
        differentiable when parameters require grad and grad mode is on), .h, .c, .ctx."""
        lstm = self.decoder.lstm
        with gate_weights_pass(self.pass_gate_weights(train), lstm.weight_ih, lstm.weight_hh):
            return self._rollout(batch, steps, feedback, train, finalize)

    def _rollout(self, batch, steps, feedback, train, finalize):
        enc, dec, store = self.encoder, self.decoder, self.store
        dev = store.device
        B, A, S = batch.batch_size, batch.a_max, steps
        bidir = enc.num_directions == 2          # train.py:197-199: hidden_size // 2 per direction
        H, E = enc.hidden_size * enc.num_directions, enc.embedding_size
        F, V = store.F, store.V
        D = dec.visual_attention_layer.linear_in_h.weight.shape[0]
        T = batch.mask.shape[1]                  # (= max(batch.lengths), or wider: a batch of fixed shapes, nav.DeviceNavBatch)
        Lpad = batch.seq.shape[1]
        training = dec.training if train is None else train
        new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
        st = RolloutState()
        st.batch, st.steps, st.dims = batch, S, (B, A, H, E, F, V, D, T)
        st.feedback = FEEDBACK[feedback]

        # dropout configuration: one seed per engine, site ids advance with the iteration
        p_dec = dec.drop.p if training else 0.0
        p_enc = enc.drop.p if training else 0.0
        if self.dropout_seed is None:
            self.dropout_seed = torch.initial_seed() & 0xFFFFFFFF
        st.drop_dec = (p_dec, self.dropout_seed, batch.row0)
        st.drop_enc = (p_enc, self.dropout_seed ^ 0x5BD1E995, batch.row0)
        # A rollout of S steps uses sites site0 .. site0 + S + 1 (x2 for the two masks of a step): the
        # next rollout starts behind them, at least 64 further on (so that S <= 62 keeps the
        # `iteration * 64` numbering the oracle tests mirror).  Identical on every data-parallel rank.
        st.site0 = self.site_next
        st.site_stride = max(64, S + 2)
        self.site_next += st.site_stride
        self.iteration += 1
        # what the kernels are given: the absolute site, or (device-side counter) 0 + the word's address
        st.site_dev = C.c_void_p(self.site_word.data_ptr()) if self.site_word is not None else None
        st.site_rel = 0 if self.site_word is not None else st.site0
        st.drop_dec += (st.site_dev, 1)
        st.drop_enc += (st.site_dev, 1)

        # ---- encoder (model.py:81-104)
        st.ctx = new(B, T, H)
        st.hs_all = new(steps + 1, B, H)
        st.cs_all = new(steps + 1, B, H)
        st.h_init, st.c_init = st.hs_all[0], st.cs_all[0]
        # (an inference rollout keeps no embedded tokens / gate tape: nothing will run backward)
        keep = training or (torch.is_grad_enabled() and any(
            p.requires_grad for p in list(enc.parameters()) + list(dec.parameters())))
        st.enc_tape = bi_encoder_tapes(B, T, E, H // 2, dev, keep) if bidir else \
            dict(emb=new(T, B, E) if keep else None, xg=new(T, B, 4 * H) if keep else None,
                 gates=new(T, B, 4 * H) if keep else None, hs=new(T + 1, B, H), cs=new(T + 1, B, H))
        etp = None if bidir else _lib.EncoderTape(*(st.enc_tape[k].data_ptr() if st.enc_tape[k] is not None else None
                                 for k in ('emb', 'xg', 'gates', 'hs', 'cs')))
        # a trainable (non-GloVe) embedding with a backward to follow: the input product is formed from the embedded
        # (train mode: dropped, model.py:86-87) tokens, not read from the cached table
        st.enc_table = not (keep and trainable_embedding(enc))
        if bidir:
            # the module's entry (model.EncoderLSTM._forward_bidirectional: sf_encoder_bilstm_fwd) on the engine's fixed
            # tapes; _backward() calls sf_encoder_bilstm_bwd.  The ctx mask is keyed on (seed + row0 mix, row b) -- the
            # numbering of the module's dropout over the assembled rows -- and the site is a device word under capture.
            p_e, seed_e, row0 = st.drop_enc[:3]
            st.drop_enc_bi = (p_e, (seed_e + 0x9E3779B1 * row0) & 0xFFFFFFFF, 0, st.site_dev, 1)
            bi_encoder_fwd(enc, batch.seq, batch.lengths_dev, T, dropout_arg(*st.drop_enc_bi), st.site_rel,
                           st.enc_table, st.enc_tape, st.ctx, st.h_init, st.c_init)
        else:
            ew = _encoder_structs(enc, table=st.enc_table)
            call('sf_encoder_lstm_fwd', byref(ew), B, Lpad, T, E, H, ptr(batch.seq),
                 ptr(batch.lengths_dev), ptr(st.ctx), ptr(st.h_init), ptr(st.c_init), byref(etp),
                 dropout_arg(*st.drop_enc), st.site_rel, *ws_args(dev))

        # ---- decode steps
        shapes = dict(t_v=(D,), q=(F,), alpha_v=(V,), xin=(2 * F,), gates=(4 * H,), c1=(H,),
                      h1=(H,), cat2=(2 * H,), t_text=(H,), alpha=(T,), h_tilde=(H,), t_a=(D,),
                      wt=(D,), r=(F,), logit=(A,))
        # one extra xin slot: step t's glue writes dropout(u_next) straight into step t+1's LSTM input
        shapes_x = dict(shapes, xin=(2 * F,))
        st.tape = {k: new(S + (1 if k == 'xin' else 0), B, *shapes_x[k]) for k in _TAPE_KEYS
                   if k not in ('h1', 'c1')}
        # hidden / cell states of all steps stacked: hs[t] is step t's h0, hs[t+1] its h1 -- the
        # batched weight-gradient products read hs[0:S] as one [S*B, H] matrix
        st.hs, st.cs = st.hs_all, st.cs_all
        st.tape['h1'], st.tape['c1'] = st.hs[1:], st.cs[1:]
        st.ended = torch.empty(B, dtype=torch.uint8, device=dev)
        # u_begin = 0 (model.py:368; the feature half of the row is written by the attention), no row has ended
        # (follower.py:380): one launch
        fill_regions((st.tape['xin'][0], 0.0), (st.ended, 0))
        st.actions = torch.empty(S, B, dtype=torch.int64, device=dev)
        st.target_used = torch.empty(S, B, dtype=torch.int64, device=dev)
        st.step_scores, st.ce_term, st.live = new(S, B), new(S, B), new(S, B)
        st.sum_cnt, st.gscale, st.loss_buf = new(S, 2), new(S), new(1)
        params = decoder_params(dec)
        all_params = list(params) + [p for p in enc.parameters()]
        st.differentiable = torch.is_grad_enabled() and any(p.requires_grad for p in all_params)
        dw = decoder_w_struct(params)
        ws = ws_args(dev)
        d_dec = _lib.Dropout(float(st.drop_dec[0]), int(st.drop_dec[1]) & 0xFFFFFFFF, int(st.drop_dec[2]), st.site_dev, 1)
        d_ptr = C.pointer(d_dec) if st.drop_dec[0] else None
        # A nav.DeviceNavBatch produces its observations ON THE DEVICE, one step ahead of the decoder,
        # from the action the glue kernel has just chosen (real student forcing: the next panorama
        # depends on a_t).  The attention of step t+1 therefore cannot ride beside tail(t); its QUERY can
        # (t_v', q' need only h1): tail(t) with tape_next but no X_next, env step, then the attention alone.
        on_device_env = hasattr(batch, 'advance')
        if on_device_env:
            batch.advance(-1)                           # slot 0 = the initial observation
        pipelined = self.pipelined and not on_device_env
        st.episode = None
        st.projected, st.projected_tables = False, None
        st.gate_rows, st.gate_rows_tables, st.gate_rows_attended = False, None, False
        st.gate_rows_recurrent = False
        # the same one-call episode for a device-resident environment (the env step inside every scoring + glue launch,
        # the attention of step t + 1 behind it): no host work between the launches of a TRAINING rollout either, and
        # the backward takes the two-stream episode path
        nav_episode = (on_device_env and self.pipelined and self.episode_call and self.fused_env_step
                       and bool(dw.visual.w_v_t))
        if (pipelined or nav_episode) and self.episode_call:
            # every per-step tensor is a stacked [S][...] array: hand step 0 to the library once
            ep = _lib.FollowerEpisode()
            ep.S, ep.B, ep.H, ep.D, ep.L, ep.A = S, B, H, D, T, A
            ep.X = store.pano(batch.vp[0], batch.view[0])
            ep.U = store.cands(batch.vp[0], batch.cand_view[0], batch.sincos[0], batch.a_num[0], A)
            ep.h_init, ep.c_init = st.h_init.data_ptr(), st.c_init.data_ptr()
            ep.ctx, ep.ctx_mask = st.ctx.data_ptr(), batch.mask.data_ptr()
            ep.tape = _lib.DecoderTape(*(st.tape[k][0].data_ptr() for k in _TAPE_KEYS))
            ep.glue = _lib.FollowerGlue(
                None, batch.target[0].data_ptr(), st.feedback, st.ended.data_ptr(),
                st.actions[0].data_ptr(), st.target_used[0].data_ptr(), st.step_scores[0].data_ptr(),
                None, 0, None, 0, st.ce_term[0].data_ptr(), st.live[0].data_ptr(),
                int(st.drop_dec[1]) ^ 0x1B873593, 0, batch.row0, st.site_dev)
            ep.drop = d_dec
            ep.step0 = st.site_rel
            ep.side_stream = None
            if nav_episode:
                st.navio0 = batch.fused_step(0)               # (sf_nav_io of step 0; the library strides it per step)
                ep.glue.nav = C.cast(C.pointer(st.navio0), C.c_void_p)
            # INFERENCE: the text attention in folded form (include/sf_hip.h, ABI 9: ctx_q / ctx_o; csrc/sf_attention.hip:
            # text_fold_body) -- the context is constant over the episode, so W_in and W_out[:, :H] are applied to it ONCE
            # and two dependent launches leave every decode step.  Nothing is taped for a backward, hence never for a
            # differentiable or train-mode rollout.
            st.text_folded = (self.fold_text and not st.differentiable and not training
                              and S > 1 and T <= 80)
            if st.text_folded:
                st.ctx_fold = new(2, B, T, H)
                ep.ctx_q, ep.ctx_o = st.ctx_fold[0].data_ptr(), st.ctx_fold[1].data_ptr()
            # ... on the projected tables of (store, decoder) where the policy has them (`project` above): the library
            # takes the two-launch chain for every step it applies to and says how many it issued
            st.projected_tables = self._projected_tables(B, T=T, A=A) if (st.text_folded and not nav_episode) else None
            st.gate_rows_tables = self._gate_rows_tables(st.projected_tables, training)
            attended = (st.gate_rows_tables is not None and self.gate_rows_attended
                        and st.gate_rows_tables['attended'] is not None)
            with projected_pass(st.projected_tables is not None), gate_rows_pass(st.gate_rows_tables is not None), \
                    gate_rows_attended_pass(attended), gate_rows_recurrent_pass(attended and self.gate_rows_recurrent):
                before, gate_before = _lib.lib.sf_projected_steps(), _lib.lib.sf_gate_rows_steps()
                att_before, rec_before = _lib.lib.sf_gate_rows_attended_steps(), _lib.lib.sf_gate_rows_recurrent_steps()
                call('sf_follower_episode_fwd', byref(dw), byref(ep), *ws)
                st.projected = _lib.lib.sf_projected_steps() > before
                st.gate_rows = _lib.lib.sf_gate_rows_steps() > gate_before
                st.gate_rows_attended = _lib.lib.sf_gate_rows_attended_steps() > att_before
                st.gate_rows_recurrent = _lib.lib.sf_gate_rows_recurrent_steps() > rec_before
            st.episode = (ep, dw)
        tapes = [] if st.episode else [_lib.DecoderTape(*(st.tape[k][t].data_ptr() for k in _TAPE_KEYS))
                                       for t in range(S)]
        panos = [] if st.episode else [store.pano(batch.vp[t], batch.view[t]) for t in range(S)]
        if pipelined and not st.episode:
            call('sf_attn_decoder_head_fwd', byref(dw), byref(panos[0]), B, H, D, ptr(st.h_init),
                 byref(tapes[0]), d_ptr, st.site_rel, *ws)
        deferred = on_device_env and self.pipelined and dw.visual.w_v_t and not st.episode
        if deferred:
            call('sf_attn_decoder_head_fwd', byref(dw), byref(panos[0]), B, H, D, ptr(st.h_init),
                 byref(tapes[0]), d_ptr, st.site_rel, *ws)
        for t in range(0 if not st.episode else S, S):
            pano = panos[t]
            cnd = store.cands(batch.vp[t], batch.cand_view[t], batch.sincos[t], batch.a_num[t], A)
            tp = tapes[t]
            h0 = st.h_init if t == 0 else st.tape['h1'][t - 1]
            c0 = st.c_init if t == 0 else st.tape['c1'][t - 1]
            glue = _lib.FollowerGlue(
                None, batch.target[t].data_ptr(), st.feedback, st.ended.data_ptr(),
                st.actions[t].data_ptr(), st.target_used[t].data_ptr(), st.step_scores[t].data_ptr(),
                st.tape['xin'][t + 1].data_ptr(), 2 * F, d_ptr, 2 * (st.site_rel + t + 1),
                st.ce_term[t].data_ptr(), st.live[t].data_ptr(),
                int(st.drop_dec[1]) ^ 0x1B873593, st.site_rel + t, batch.row0, st.site_dev)
            navio = None
            if deferred and self.fused_env_step:        # env.step + observe in the scoring + glue launch
                navio = batch.fused_step(t)
                glue.nav = C.cast(C.pointer(navio), C.c_void_p)
            if pipelined or deferred:
                nxt = t + 1 < S
                call('sf_attn_decoder_tail_fwd', byref(dw), byref(cnd), B, H, D, T, None, ptr(h0),
                     ptr(c0), ptr(st.ctx), ptr(batch.mask), None, byref(tp), byref(glue), d_ptr,
                     st.site_rel + t, byref(panos[t + 1]) if nxt and not deferred else None,
                     byref(tapes[t + 1]) if nxt else None, *ws)
            else:
                call('sf_attn_decoder_fwd', byref(dw), byref(pano), byref(cnd), B, H, D, T, None,
                     ptr(h0), ptr(c0), ptr(st.ctx), ptr(batch.mask), None, byref(tp), byref(glue),
                     d_ptr, st.site_rel + t, *ws)
            if on_device_env:                           # env.step + observe + teacher for step t + 1
                if navio is None:
                    batch.advance(t, st.actions[t], st.ended)
                if deferred and t + 1 < S:              # the attention of step t + 1 over the panorama just chosen
                    call('sf_attn_decoder_attend_fwd', byref(panos[t + 1]), B, byref(tapes[t + 1]), d_ptr,
                         st.site_rel + t + 1, *ws)
        call('sf_reduce_terms', ptr(st.ce_term), ptr(st.live), S, B, ptr(st.sum_cnt), ws[2])
        st.logits = st.tape['logit']
        st.h, st.c = st.tape['h1'][S - 1], st.tape['c1'][S - 1]
        st.all_params = all_params
        if not finalize:            # a row shard of a larger batch: the caller combines sum_cnt tables
            return st               # and calls finish(st, total)
        if self.group is not None:
            # global per-step normaliser so that the sharded loss equals the reference's batch mean
            # (a collective point: under a segmented capture the graph is cut here, runtime.TrainingGraph)
            table, grp = st.sum_cnt, self.group
            self._collective(lambda: torch.distributed.all_reduce(table, group=grp))
        return self.finish(st)

    collective_hook = None        # runtime.TrainingGraph (segmented): takes the host action of a collective point

    def _collective(self, action):
        if self.collective_hook is not None:
            self.collective_hook(action)
        else:
            action()

    def run(self, batch, steps, feedback='argmax', train=None, backward=False, while_running=None):
        """`rollout` (and, with backward=True, `loss.backward()`) + the fault check of the persistent encoder
        launches: ONE host sync, and the fault protocol of DESIGN.md (runtime.reissue_per_step) -- the SAME rollout,
        same dropout / sampling sites, again with the per-step encoder kernels (SF_ENC_PER_STEP), after zeroing the
        gradients the poisoned backward accumulated.  Under a process group the decision is taken on the MAX of all
        ranks' fault words, so every rank re-issues together; gradient buckets the poisoned backward had launched are
        waited for and re-armed (`BucketedGrads.abort`) first.
        `while_running()`: host work the caller wants done between the issue and the sync (the next minibatch)."""
        dev = self.store.device
        site, it = self.site_next, self.iteration
        group = self.group if self.group is not None and collectives_on(self.group) else None

        def issue():
            st = self.rollout(batch, steps, feedback, train)
            if backward:
                st.loss.backward()
            return st

        st = issue()
        if while_running is not None:
            while_running()
        bits = fault_bits(dev, group)
        if bits:
            if backward:
                # the poisoned backward has already launched its gradient buckets (on every rank alike): let them
                # land before the buffer is zeroed, and re-arm the buckets for the re-issued backward
                if self.grad_sync is not None:
                    self.grad_sync.abort()
                for p_ in st.all_params:
                    if p_.grad is not None:
                        p_.grad.zero_()
            self.site_next, self.iteration = site, it
            st = reissue_per_step(self.encoder, self, dev, 'a rollout', issue, bits, group)
        return st

    def finish(self, st, total=None):
        """Second half of `rollout(..., finalize=False)`: turns the per-step (CE sum, live count) table
        into the loss.  `total` = the table summed over every row shard of the batch (what the
        data-parallel all-reduce produces across GPUs); with it the shard's loss IS the whole batch's
        loss (follower.py:481: per-step mean over the non-ignored rows of the full batch) and its
        backward() contributes exactly this shard's share of the batch gradient."""
        if total is not None:
            st.sum_cnt = total
        call('sf_loss_finalize', ptr(st.sum_cnt), st.steps, ptr(st.loss_buf), ptr(st.gscale), stream())
        if st.differentiable:
            st.loss = _RolloutLossFn.apply(self, st, *st.all_params)
        else:
            st.loss = st.loss_buf.reshape(())
        return st

    def _baked_pointers(self, gate_weights='fp32', projected=False, gate_rows=False, attended=False):
        """Every weight-side device pointer a captured rollout bakes into its hipGraph: the parameters
        and their derived copies (transposed layouts, the encoder's [vocab,4H] table, with
        gate_weights = 'bf16' the packed images of the decoder LSTM's weights).  Building the
        structs also refreshes stale derived copies IN PLACE, on the current stream."""
        enc = self.encoder
        if enc.num_directions == 2:
            e2d = enc.encoder2decoder
            ew = b''.join(bytes(_encoder_structs(enc, direction=d)) for d in (0, 1)) + \
                repr((e2d.weight.data_ptr(), e2d.bias.data_ptr(), transposed(e2d.weight).data_ptr())).encode()
        else:
            ew = bytes(_encoder_structs(enc))
        dw = decoder_w_struct(decoder_params(self.decoder))
        packed = b''
        if gate_weights == 'bf16':
            lstm = self.decoder.lstm
            packed = repr(tuple(t.data_ptr() for t in register_bf16_weights(lstm.weight_ih, lstm.weight_hh))).encode()
        tables = b''
        if projected:
            # (refreshed in place here when a weight they depend on changed; re-allocated or gone: the bytes differ)
            hit = self.store.projected(self.decoder, build=False)
            tables = b'projected' + (bytes(hit['struct']) if hit is not None else b'')
        if gate_rows:
            # (`attended`: whether the CAPTURED rollout ran on the attended half's table.  Only then is that table part of
            # what the graph reads: a table another engine added to the entry since is none of this graph's business, and
            # a refresh here never adds one -- FeatureStore.gate_rows grows the entry only where `build` is true)
            hit = self.store.gate_rows(self.decoder, build=False, **({} if attended else {'attended': False}))
            tables += b'gate_rows' + (bytes(hit['struct']) if hit is not None else b'')
            if attended:
                att = hit['attended'] if hit is not None else None
                tables += b'attended' + (bytes(att['struct']) if att is not None else b'')
        return ew + bytes(dw) + packed + tables

    @contextlib.contextmanager
    def _capture_policy(self):
        """What `project = 'auto'` means inside capture(): the rollouts issued here build the projected tables."""
        prev, self._capturing = self._capturing, True
        try:
            yield
        finally:
            self._capturing = prev

    def _guarded(self, graph_replay, projected=False, gate_rows=False, attended=False):
        mode = self._gate_weights          # (the captured rollouts ran train=False under no_grad: this mode, for good)
        baked = self._baked_pointers(mode, projected, gate_rows, attended)

        def replay():
            # weights updated since capture (optimizer.step, load_state_dict)?  Their derived copies are
            # rebuilt in place here, ahead of the replay on the same stream, so the graph reads current
            # data everywhere.  A MOVED tensor cannot be patched into the graph: refuse.
            if self._baked_pointers(mode, projected, gate_rows, attended) != baked:
                raise WeightsMoved('a weight (or one of its cached layouts) moved since this rollout was '
                                   'captured; capture() again')
            graph_replay()
        return replay

    def capture(self, batch, steps, feedback='argmax'):
        """hipGraph of one inference rollout (eval mode, no autograd): returns (replay, state).
        `replay()` re-runs encoder + `steps` decode steps on the captured buffers; the state's
        tensors (.actions, .logits, .loss_buf, ...) are overwritten by every replay.

        The graph holds raw device pointers of the weights AND of their cached derived copies
        (`runtime.transposed`, the encoder's embedding x W_ih^T table).  Those copies live in
        persistent buffers that are refreshed in place, and `replay()` refreshes them first when a
        weight's version changed, so replays after `optimizer.step()` / `load_state_dict` use the new
        weights; if a weight tensor itself was re-allocated, `replay()` raises and the rollout must be
        captured again.  Dropout sites are fixed at capture time: a captured TRAINING rollout would
        replay one mask forever, which is why only inference is captured here."""
        # `sample` feedback: the sampling stream of a replay is a device word replay() writes first (kernel arguments are
        # frozen in a graph): every replay draws new actions (sf_follower_glue.sample_site_dev)
        sampled = feedback == 'sample'
        ctl = torch.zeros(4, dtype=torch.int32, device=self.store.device) if sampled else None
        with torch.no_grad(), self._capture_policy():
            self.rollout(batch, steps, feedback, train=False)          # warm-up: allocations, caches, projected tables
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            ensure_workspace(side, self.store.device)                  # (created and zero-filled OUTSIDE the graph)
            side.wait_stream(torch.cuda.current_stream())
            keep = (self.site_next, self.iteration)
            self.site_word = ctl[0:1] if sampled else None
            try:
                with torch.cuda.stream(side):
                    with graph_capture(graph, side):
                        st = self.rollout(batch, steps, feedback, train=False)
            finally:
                self.site_word = None
            if sampled:
                self.site_next, self.iteration = keep                  # (the capture ran nothing)
            torch.cuda.current_stream().wait_stream(side)
        # (the graph bakes the capture stream's workspace -- runtime.workspace is keyed on the stream handle -- so the
        # stream lives as long as the state: a recycled handle would hand the same scratch to someone else)
        st.capture_stream = side

        def graph_replay():
            if sampled:
                call('sf_store_u32x4', C.c_void_p(ctl.data_ptr()), int(self.site_next) & 0xFFFFFFFF, 0, 0, 0, stream())
                st.site0 = self.site_next
                self.site_next += st.site_stride
                self.iteration += 1
            graph.replay()
        return self._guarded(graph_replay, st.projected, st.gate_rows, st.gate_rows_attended), st

    def capture_training(self, batch, steps, feedback='sample', optimizers=(), zero=None):
        """hipGraph of ONE WHOLE TRAINING ITERATION (follower.py:1001-1020 + train.py:263-268): zero the gradients,
        rollout in train mode (dropout on, `feedback` as given), BPTT, `optimizer.step()` for every optimizer
        (optim.FusedAdam).  Returns a runtime.TrainingGraph; `.replay()` is one iteration, `.state` the rollout state
        its replays overwrite.  Runs one eager iteration first (a real training step).

        Every replay draws fresh dropout masks / samples and takes the next Adam step: sites and step counters are
        device words the graph reads (sf_dropout.site_dev, sf_adam_step_dev), numbered exactly like the eager loop's.
        Single process only (a gradient all-reduce cannot live in the graph); pre-drawn observations or a device-resident
        environment (nav.DeviceNavBatch).  A bidirectional encoder is captured in the single-process form only; the
        segmented data-parallel capture takes a unidirectional one."""
        from .runtime import TrainingGraph
        opts = list(optimizers)
        if self.group is not None or self.grad_sync is not None:
            if self.encoder.num_directions == 2:
                raise NotImplementedError('capture_training: a data-parallel iteration with a bidirectional encoder '
                                          'runs eagerly')
            return self._capture_training_dp(batch, steps, feedback, opts, zero)

        def body():
            if zero is not None:
                zero.zero()
            else:
                for o in opts:
                    o.zero_grad()
            st = self.rollout(batch, steps, feedback, train=True)
            st.loss.backward()
            for o in opts:
                o.step()
            return st
        return TrainingGraph(self, body, opts, self.store.device)

    def _capture_training_dp(self, batch, steps, feedback, opts, zero):
        """The DATA-PARALLEL iteration as replayed SEGMENTS (runtime.TrainingGraph, segmented): a collective cannot
        live in the graph (gloo stages through the host; RCCL's kernels belong to the process group's own stream), so the
        capture is CUT at every collective point -- the all-reduce of the per-step (CE sum, count) table behind the
        forward, the start of each gradient bucket's all-reduce behind the launches that complete it, the wait in front
        of the optimizers -- and a replay is: segment, host action, segment, ...: the launches of an iteration are still
        issued as a handful of graph launches instead of ~400 kernel launches, the collectives keep the order and the
        overlap of the eager loop (each is started behind exactly the work that precedes it on the replay stream; the
        persistent encoder backward runs in the segment BEHIND the 40 MB bucket's start).  Same sites, same Adam steps,
        same numbers as the eager data-parallel loop (tests/test_gpu_dataparallel.py)."""
        from .runtime import TrainingGraph
        sync = self.grad_sync
        if sync is None:
            raise ValueError('a data-parallel capture needs engine.grad_sync (dp.BucketedGrads: the buffer the '
                             'all-reduces work on)')
        zero = zero if zero is not None else sync
        dev = self.store.device

        def body():
            zero.zero()
            with torch.no_grad():                       # (the backward is called directly: every launch on this thread)
                st = self.rollout(batch, steps, feedback, train=True)
                self._backward(st, torch.ones((), device=dev))
            sync.wait()
            for o in opts:
                o.step()
            return st
        return TrainingGraph(self, body, opts, dev, segmented=(sync,))

    def capture_sharded(self, shards, steps, feedback='argmax'):
        """Runs the row shards of ONE batch as concurrent chains (inference): one hipGraph per
        shard, replayed on its own stream.  Samples never interact in the forward pass, and at batch
        100 every stage of the chain is latency-bound with most of the 256 CUs idle, so two
        half-batch chains overlap; the per-step (CE sum, live count) tables are added before the loss
        is finalised, exactly like the data-parallel path does across GPUs.  (One graph per stream:
        branches of a single hipGraph do run concurrently on ROCm 7.2 -- tools/graph_branch_probe.py --
        but every fork / join between them costs several microseconds.)  Returns (replay, states,
        loss_buf)."""
        dev = self.store.device
        streams = [torch.cuda.Stream() for _ in shards]
        graphs, states = [], []
        with torch.no_grad(), self._capture_policy():
            for sh, s in zip(shards, streams):
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    self.rollout(sh, steps, feedback, train=False)          # warm-up on this stream
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with graph_capture(g, s):
                        states.append(self.rollout(sh, steps, feedback, train=False, finalize=False))
                graphs.append(g)
            torch.cuda.synchronize()
        total = torch.empty(steps, 2, device=dev)
        loss_buf = torch.empty(1, device=dev)
        gscale = torch.empty(steps, device=dev)

        def replay_all():
            cur = torch.cuda.current_stream()
            for s, g in zip(streams, graphs):
                s.wait_stream(cur)
                with torch.cuda.stream(s):
                    g.replay()
            for s in streams:
                cur.wait_stream(s)
            total.copy_(states[0].sum_cnt)
            for st in states[1:]:
                call('sf_add_f32', ptr(total), ptr(st.sum_cnt), total.numel(), stream())
            call('sf_loss_finalize', ptr(total), steps, ptr(loss_buf), ptr(gscale), stream())

        return self._guarded(replay_all, any(st.projected for st in states), any(st.gate_rows for st in states),
                             any(st.gate_rows_attended for st in states)), states, loss_buf

    # ------------------------------------------------------------------------------ backward
    def _backward(self, st, dloss):
        """BPTT.  Per step only the DATA gradients are formed (sequential dependency); every
        weight gradient is one product over all S*B stacked rows at the end (sf_attn_decoder_wgrad),
        accumulated in place into param.grad."""
        enc, dec, store = self.encoder, self.decoder, self.store
        batch, S = st.batch, st.steps
        B, A, H, E, F, V, D, T = st.dims
        dev = store.device
        new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
        gscale = st.gscale * dloss.to(torch.float32)        # d loss / d step-loss, per step
        params = decoder_params(dec)
        dw, dg = decoder_w_struct(params), decoder_w_struct(params, grad=True)
        gshapes = dict(dgates=(4 * H,), dpre=(H,), dt_text=(H,), dt_v=(D,), dq=(F,), dwt=(D,),
                       dta=(D,), dr=(F,), dc=())
        gkeys = ('dgates', 'dpre', 'dt_text', 'dt_v', 'dq', 'dwt', 'dta', 'dr', 'dc')
        gt = {k: new(S, B, *gshapes[k]) for k in gkeys}
        dlogit = new(B, A)
        dh_a, dc_a, dh_b, dc_b = new(B, H), new(B, H), new(B, H), new(B, H)
        dctx = torch.zeros(B, T, H, device=dev, dtype=torch.float32)
        ws = ws_args(dev)
        d_dec = _lib.Dropout(float(st.drop_dec[0]), int(st.drop_dec[1]) & 0xFFFFFFFF, int(st.drop_dec[2]), st.site_dev, 1)
        d_ptr = C.pointer(d_dec) if st.drop_dec[0] else None
        dh1 = dc1 = None
        if st.episode is not None:
            ep, _ = st.episode
            # d[wc ; h1_drop] and d(score) of every step: the context gradient is formed once after
            # the loop instead of a read-modify-write of [B,T,H] per step
            gt_dcat2, gt_ds, gt_dh1d = new(S, B, 2 * H), new(S, B, T), new(S, B, H)
            gt0e = _lib.DecoderGTape(*(gt[k].data_ptr() for k in gkeys), gt_dcat2.data_ptr(), gt_ds.data_ptr(),
                                     gt_dh1d.data_ptr())
            # second stream: the scoring / text-attention backward of step t-1 runs beside the LSTM /
            # visual backward of step t (not under stream capture: eager issue only)
            # (under stream capture only with a side stream that already exists: probing one launches timed kernels)
            if self.two_stream_backward and (self._side_stream is not None or not torch.cuda.is_current_stream_capturing()):
                if self._side_stream is None:
                    self._side_stream = concurrent_stream(dev)
                ep.side_stream = self._side_stream.cuda_stream
            else:
                ep.side_stream = None
            which = C.c_int(0)
            call('sf_follower_episode_bwd', byref(dw), byref(ep), byref(gt0e), ptr(gscale), ptr(dlogit),
                 ptr(dh_a), ptr(dc_a), ptr(dh_b), ptr(dc_b), ptr(dctx), byref(which), *ws)
            dh1, dc1 = (dh_b, dc_b) if which.value else (dh_a, dc_a)
        for t in range(S - 1 if st.episode is None else -1, -1, -1):
            pano = store.pano(batch.vp[t], batch.view[t])
            cnd = store.cands(batch.vp[t], batch.cand_view[t], batch.sincos[t], batch.a_num[t], A)
            tp = _lib.DecoderTape(*(st.tape[k][t].data_ptr() for k in _TAPE_KEYS))
            gtp = _lib.DecoderGTape(*(gt[k][t].data_ptr() for k in gkeys), None, None, None)
            call('sf_follower_glue_bwd', B, A, ptr(st.tape['logit'][t]), ptr(st.target_used[t]),
                 ptr(gscale[t:t + 1]), ptr(dlogit), ws[2])
            call('sf_attn_decoder_bwd', byref(dw), None, byref(pano), byref(cnd), B, H, D, T,
                 ptr(st.hs[t]), ptr(st.cs[t]), ptr(st.ctx), byref(tp), byref(gtp), ptr(dlogit),
                 ptr(dh1), ptr(dc1), ptr(dh_a), ptr(dc_a), ptr(dctx), d_ptr, st.site_rel + t, *ws)
            dh1, dc1 = dh_a, dc_a
            dh_a, dc_a, dh_b, dc_b = dh_b, dc_b, dh_a, dc_a
        # data parallelism: dp.BucketedGrads laid out as dp.follower_buckets -- each bucket's all-reduce is
        # launched from here, behind the launches that complete it
        sync = self.grad_sync
        tp0 = _lib.DecoderTape(*(st.tape[k].data_ptr() for k in _TAPE_KEYS))
        gt0 = _lib.DecoderGTape(*(gt[k].data_ptr() for k in gkeys), None, None, None)
        # the decoder's weight gradients (a few large products over the stacked rows: matrix-core
        # work) and the encoder's backward through time (80 dependent, latency-bound steps) are
        # independent: issued on two streams they overlap
        overlap = self.two_stream_backward and (self._side_stream is not None or not torch.cuda.is_current_stream_capturing())
        if overlap:
            side = self._side_stream
            if side is None:
                side = self._side_stream = concurrent_stream(dev)
            side.wait_stream(torch.cuda.current_stream())
            self._open_forks = [side]                    # (a segmented capture joins / re-opens these at its cuts)
        # (Measured in round 5 by wall clock: the encoder first, the two latency-bound pieces side by side, a third stream
        # and chunked weight gradients ("Retired experiments") are all equal or slower than this order; what shortened the tail was fewer launches,
        # gemm_tn_group.  The many-row weight-gradient tiles -- 512 threads x 188 VGPRs, 96 KB LDS -- cannot sit beside the
        # persistent encoder backward's 256-VGPR workgroup on a CU.  NOTE: rocprofv3 --kernel-trace serialises the queues;
        # its timelines show no overlap at all and must not be read for concurrency; DESIGN.md, "Retired experiments".)
        try:
            if overlap:
                self._issue_wgrad(side, dw, dg, params, S * B, H, D, F, st, tp0, gt0, dev, sync)
            else:
                self._decoder_wgrad(dw, dg, params, S * B, H, D, F, st, tp0, gt0, wgrad_ws_args(dev), sync)
            if enc.num_directions == 2:
                bi_encoder_bwd(enc, batch.seq, batch.lengths_dev, T, dropout_arg(*st.drop_enc_bi), st.site_rel,
                               st.enc_table, st.enc_tape, st.h_init, dctx, dh1, dc1)
            else:
                etp = _lib.EncoderTape(*(st.enc_tape[k].data_ptr() for k in ('emb', 'xg', 'gates', 'hs', 'cs')))
                ew = _encoder_structs(enc, table=st.enc_table)
                eg = _encoder_structs(enc, grad=True, seq=None if st.enc_table else batch.seq)
                call('sf_encoder_lstm_bwd', byref(ew), byref(eg), B, T, E, H, ptr(batch.lengths_dev),
                     ptr(st.h_init), ptr(dctx), ptr(dh1), ptr(dc1), byref(etp), dropout_arg(*st.drop_enc),
                     st.site_rel, *ws)
            if sync is not None:
                sync.launch(2)                       # encoder gradients: complete behind sf_encoder_lstm_bwd
            if overlap:
                torch.cuda.current_stream().wait_stream(side)
        finally:
            self._open_forks = []        # (also when the backward raises: a later segmented capture must not join stale forks)

    def _issue_wgrad(self, side, dw, dg, params, M, H, D, F, st, tp0, gt0, dev, sync):
        """The decoder's weight gradients on the side stream (which already waits for the backward through time)."""
        with torch.cuda.stream(side):
            self._decoder_wgrad(dw, dg, params, M, H, D, F, st, tp0, gt0, wgrad_ws_args(dev), sync)

    @staticmethod
    def _decoder_wgrad(dw, dg, params, M, H, D, F, st, tp0, gt0, ws, sync):
        """sf_attn_decoder_wgrad on the current stream.  With a gradient-bucket sync it is two calls -- the two LSTM
        products + bias sums (the 40 MB gradient bucket), then the other decoder weights -- and each part's all-reduce is
        launched behind it."""
        if sync is None:
            call('sf_attn_decoder_wgrad', byref(dw), byref(dg), M, H, D, F, ptr(st.hs), byref(tp0), byref(gt0), *ws)
            return
        g_lstm, g_rest = _lib.DecoderW(), _lib.DecoderW()
        g_lstm.lstm = dg.lstm
        g_rest.visual, g_rest.text, g_rest.action = dg.visual, dg.text, dg.action
        call('sf_attn_decoder_wgrad', byref(dw), byref(g_lstm), M, H, D, F, ptr(st.hs), byref(tp0), byref(gt0), *ws)
        sync.launch(0)
        call('sf_attn_decoder_wgrad', byref(dw), byref(g_rest), M, H, D, F, ptr(st.hs), byref(tp0), byref(gt0), *ws)
        sync.launch(1)
