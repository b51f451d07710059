"""Seq2SeqAgent / Seq2SeqSpeaker with the reference's interface (follower.py:261-1035,
speaker.py:34-410) on top of the HIP modules, for environments that hand out the reference's
observation dictionaries (env.py:775-795: 'feature', 'action_embedding', 'adj_loc_list',
'teacher', 'instr_encoding', ...).  The per-step arithmetic -- decoder step, masking,
cross-entropy, action choice, u_prev gather -- runs through the C ABI; the loop, the trajectory
book-keeping and the simulator calls stay in Python exactly where the reference has them.

When observations are available in index form, `FollowerEngine` / `SpeakerEngine` are the fast
path; this module is the drop-in path.  Beam search, state-factored search and the speaker's beam search
(follower.py:541-980, speaker.py:211-318) live in search.py and run on index-form observations.

The baseline agents (StopAgent, ShortestAgent, RandomAgent; follower.py:197-259) have no network: a host path over the
environment's own calls, and a device path that is one sf_nav_walk launch per rollout.
"""
import ctypes as C
import json
import random
import sys

import numpy as np
import torch

from . import _lib
from ._lib import call
from .lazydict import LazyDict
from .follower import batch_instructions_from_encoded, FEEDBACK, PAD, EOS, BOS
from .runtime import (ptr, stream, require_gpu, cands_dense, gc_paused, WeightsMoved, take_fault, fault_views, fault_bits,
                      per_step_kernels, reissue_per_step)
from .sweeps import epoch_minibatches

byref = C.byref


def path_element_from_observation(ob):
    return (ob['viewpoint'], ob['heading'], ob['elevation'])           # follower.py utility


class _FollowerGlueFn(torch.autograd.Function):
    """follower.py:476-505 on dense tensors: returns (ce_term [B], live [B]); a_t, per-step scores
    and u_next are side outputs.  backward: softmax - onehot through sf_follower_glue_bwd."""

    @staticmethod
    def forward(ctx, logit, all_u, is_valid, target, feedback, ended_dev, sample_cfg):
        B, A = logit.shape
        dev = logit.device
        masked = logit.detach().clone()
        new = lambda *s, dt=torch.float32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
        a_t, tused = new(B, dt=torch.int64), new(B, dt=torch.int64)
        score, ce, live = new(B), new(B), new(B)
        u_next = new(B, all_u.shape[2])
        cnd = cands_dense(all_u)
        g = _lib.FollowerGlue(is_valid.data_ptr(), target.data_ptr(), feedback, ended_dev.data_ptr(),
                              a_t.data_ptr(), tused.data_ptr(), score.data_ptr(), u_next.data_ptr(),
                              all_u.shape[2], None, 0, ce.data_ptr(), live.data_ptr(),
                              sample_cfg[0], sample_cfg[1], 0)
        call('sf_follower_glue_fwd', byref(cnd), B, ptr(masked), byref(g), stream())
        ctx.save_for_backward(masked, tused)
        ctx.mark_non_differentiable(live, a_t, score, u_next, masked)
        return ce, live, a_t, score, u_next, masked

    @staticmethod
    def backward(ctx, dce, *_):
        masked, tused = ctx.saved_tensors
        B, A = masked.shape
        one = torch.ones(1, device=masked.device)
        dlogit = torch.empty_like(masked)
        call('sf_follower_glue_bwd', B, A, ptr(masked), ptr(tused), ptr(one), ptr(dlogit), stream())
        return dlogit * dce.reshape(B, 1), None, None, None, None, None, None


class BaseAgent(object):
    """follower.py:107-192."""

    def __init__(self, env, results_path):
        self.env = env
        self.results_path = results_path
        random.seed(1)
        self.results = {}
        self.losses = []

    def write_results(self):
        results = {k: {'instr_id': v['instr_id'], 'trajectory': v['trajectory']}
                   for k, v in self.results.items()}
        with open(self.results_path, 'w') as f:
            json.dump(results, f)

    def rollout(self):
        raise NotImplementedError

    @staticmethod
    def get_agent(name):
        return globals()[name + 'Agent']                               # follower.py:131-133

    def test(self):
        self.env.reset_epoch()
        self.losses = []
        self.results = {}
        looped = False
        while True:                                                    # follower.py:145-188
            for result in self.rollout():
                if result['instr_id'] in self.results:
                    looped = True
                else:
                    self.results[result['instr_id']] = result
            if looped:
                break
        return self.results


class _TableAgent(BaseAgent):
    """What the three baseline agents (follower.py:197-259) share: a policy that is a table look-up, walked either on
    the host over env.reset / observe / step, or -- when the environment yields a navigation table on the device, the
    way Seq2SeqAgent._device_table finds one -- as ONE sf_nav_walk launch (nav.NavTable.walk) with one download and one
    host sync per rollout().  Both paths give == results."""
    walk_policy = None           # _lib.SF_WALK_*
    walk_steps = 1               # S of the launch: the most actions an episode takes
    nav_table = None
    store = None
    auto_device_env = True

    def use_device_env(self, nav_table):
        self.nav_table = nav_table

    def _device_table(self):
        """The navigation table to walk on, or None for the host path: the one given to use_device_env, else (auto) the
        current env's own when it carries a feature store and no host table -- and only a table that is on a GPU."""
        nav = self.nav_table
        if nav is None:
            if not self.auto_device_env or getattr(self.env, 'host_table', 1) is not None or not hasattr(self.env, 'graphs'):
                return None
            feats = getattr(self.env, 'image_features_list', None) or [None]
            store = self.store if self.store is not None else getattr(feats[0], 'store', None)
            if store is None:
                return None
            from .nav import table_for
            nav = table_for(self.env, store)
        return nav if nav.device.type == 'cuda' else None

    def _first_actions(self, nav, rows, views):
        return None

    def walk_inputs(self, nav, items):
        """Host side of a device walk of `items`: start states, and what the policy reads (RandomAgent draws here)."""
        rows, views = nav.start_states(items)
        hop, base = nav.hop_rows(items) if self.walk_policy == _lib.SF_WALK_SHORTEST else (None, None)
        return dict(rows=rows, views=views, first_action=self._first_actions(nav, rows, views), hop=hop, base=base)

    def walk_error(self):
        """The host path's exception for a row sf_nav_walk refused."""
        return RuntimeError('sf_nav_walk: a start view outside the table')

    def _rollout_on_device(self, nav):
        self.env.reset()
        items = list(self.env.batch)
        out = nav.walk(self.walk_policy, self.walk_steps, **self.walk_inputs(nav, items))
        S, B = self.walk_steps, len(items)
        host = torch.empty(2 * (S + 1) * B + B + 1, dtype=torch.int32).pin_memory()
        host.copy_(torch.cat([out['row'].reshape(-1), out['view'].reshape(-1), out['n_steps'], out['err']]),
                   non_blocking=True)
        torch.cuda.current_stream().synchronize()                      # the one host sync of the rollout
        h = host.numpy()
        if h[-1]:
            raise self.walk_error()
        n = (S + 1) * B
        return nav.walk_results(items, h[:n].reshape(S + 1, B), h[n:2 * n].reshape(S + 1, B), h[2 * n:2 * n + B])

    def rollout(self):
        nav = self._device_table()
        return self._rollout_on_device(nav) if nav is not None else self._rollout_on_host()


class StopAgent(_TableAgent):
    """follower.py:197-207: an agent that does not move."""
    walk_policy, walk_steps = _lib.SF_WALK_STOP, 1

    def _rollout_on_host(self):
        obs = self.env.observe(self.env.reset())
        return [{'instr_id': ob['instr_id'], 'trajectory': [path_element_from_observation(ob)]} for ob in obs]


class RandomAgent(_TableAgent):
    """follower.py:210-243: a random first direction, then candidate 1 ("straight on") for four more viewpoint steps,
    then stop.  The first action comes from numpy's GLOBAL stream, `np.random.randint(len(adj) - 1) + 1`, one draw per
    observation in observation order, on both paths."""
    walk_policy, walk_steps = _lib.SF_WALK_RANDOM, _lib.SF_WALK_RANDOM_MOVES + 1

    def _rollout_on_host(self):
        env = self.env
        ws = env.reset()
        obs = env.observe(ws)
        traj = [{'instr_id': ob['instr_id'], 'trajectory': [path_element_from_observation(ob)]} for ob in obs]
        for t in range(_lib.SF_WALK_RANDOM_MOVES):                     # (the stop behind them is a no-op: not walked)
            if t == 0:
                actions = [np.random.randint(len(ob['adj_loc_list']) - 1) + 1 for ob in obs]
            else:
                for ob in obs:
                    assert len(ob['adj_loc_list']) > 1
                actions = [1] * len(obs)
            ws = env.step(ws, actions, obs)
            obs = env.observe(ws)
            for tr, ob in zip(traj, obs):
                tr['trajectory'].append(path_element_from_observation(ob))
        return traj

    def _first_actions(self, nav, rows, views):
        from .nav import V
        a_num = nav.host['a_num'][rows.astype(np.int64) * V + views].tolist()
        return np.array([np.random.randint(n - 1) + 1 for n in a_num], np.int32)

    def walk_error(self):
        return AssertionError('RandomAgent: a dead end on the way')


class ShortestAgent(_TableAgent):
    """follower.py:245-259: the teacher's route to the goal, at most 20 actions; the last observation is dropped (the
    stop is a no-op, so the end state would appear twice)."""
    walk_policy, walk_steps = _lib.SF_WALK_SHORTEST, 20

    def _rollout_on_host(self):
        all_obs, _ = self.env.shortest_paths_to_goals(self.env.reset(), self.walk_steps)
        return [{'instr_id': obs[0]['instr_id'], 'trajectory': [path_element_from_observation(ob) for ob in obs[:-1]]}
                for obs in all_obs]


class Seq2SeqAgent(BaseAgent):
    """follower.py:261-1035 (greedy / teacher / sample rollouts, scoring, train, save/load)."""
    feedback_options = ['teacher', 'argmax', 'sample']

    def __init__(self, env, results_path, encoder, decoder, episode_len=10, beam_size=1,
                 reverse_instruction=True, max_instruction_length=80):
        super().__init__(env, results_path)
        self.encoder, self.decoder = encoder, decoder
        self.episode_len = episode_len
        self.losses = []
        self.beam_size = beam_size
        self.reverse_instruction = reverse_instruction
        self.max_instruction_length = max_instruction_length
        self.feedback = 'argmax'
        self.loss = 0
        self._sample_seed = torch.initial_seed() & 0xFFFFFFFF
        self._sample_count = 0
        self.store = None          # features.FeatureStore: enables the index-form search procedures
        self.nav_table = None      # nav.NavTable: rollouts step the environment ON THE DEVICE
        self._engine = None
        # An environment that carries its feature store and no host copy of the table (compat.env.R2RBatch, what
        # the reference's train.py builds through the bare-name shim) can only be walked on the device: rollouts
        # then use nav.table_for(env, store) of whatever env is current (train.py switches agent.env between
        # the training and the validation environments, train.py:97, 111).
        self.auto_device_env = True

    def use_device_env(self, nav_table):
        """Opt in to device-resident navigation (nav.py): `_rollout_with_loss` -- and with it `train`,
        `test` and `rollout` -- then runs the whole episode with one host sync instead of a D2H copy
        plus Python env.step / observe per step.  Needs `self.store`; the env must be the
        R2RIndexEnv the table was built from.  The result dictionaries carry instr_id / trajectory /
        actions / scores (no per-step 'observations': nothing observes on the host any more)."""
        from .follower import FollowerEngine
        if self.store is None:
            raise RuntimeError('use_device_env needs a features.FeatureStore (agent.store)')
        self.nav_table = nav_table
        self._engine = FollowerEngine(self.encoder, self.decoder, self.store)
        self._engine.dropout_seed = self._sample_seed ^ 0x1B873593
        self._engine.gate_weights = self.gate_weights

    # Weight storage of the decoder LSTM's gate product in INFERENCE passes: 'fp32' (default) or 'bf16' (FollowerEngine.
    # gate_weights; include/sf_hip.h: sf_gate_product_bf16_weights).  Handed to every engine and search step the agent
    # builds -- test on the device environment, beam_search, state_factored_search, route scoring; training passes ignore
    # it.  The per-step host loop over the decoder MODULE (no store / device environment) is not covered.
    _gate_weights = 'fp32'

    @property
    def gate_weights(self):
        return self._gate_weights

    @gate_weights.setter
    def gate_weights(self, mode):
        from .runtime import check_gate_weights
        self._gate_weights = check_gate_weights(mode)
        for name in ('_engine', '_score_engine'):
            eng = self.__dict__.get(name)
            if eng is not None:
                eng.gate_weights = mode

    def _env_store(self):
        """The feature store the current env was built over (compat.env.MeanPooledImageFeatures.store), if any."""
        feats = getattr(self.env, 'image_features_list', None) or [None]
        return getattr(feats[0], 'store', None)

    def _device_table(self):
        """The navigation table to roll out on, or None for the per-step host loop: the one given to
        use_device_env, else (auto) the current env's own when it can only be walked on the device."""
        if self.nav_table is not None:
            return self.nav_table
        if not self.auto_device_env or getattr(self.env, 'host_table', 1) is not None or not hasattr(self.env, 'graphs'):
            return None
        if self.store is None:
            self.store = self._env_store()
        if self.store is None:
            return None
        from .follower import FollowerEngine
        from .nav import table_for
        if self._engine is None:
            self._engine = FollowerEngine(self.encoder, self.decoder, self.store)
            self._engine.dropout_seed = self._sample_seed ^ 0x1B873593
            self._engine.gate_weights = self.gate_weights
        return table_for(self.env, self.store)

    def _rollout_on_device(self, table=None, reissue=False):
        """One rollout on the device-resident environment (`FollowerEngine.run`: the fault protocol of DESIGN.md
        inside).  reissue=True (train(): a fault raised by the BACKWARD): the current minibatch again, per-step kernels."""
        from .nav import DeviceNavBatch
        if not reissue:
            self.env.reset(sort=True)
        nav = table if table is not None else self.nav_table
        items = list(self.env.batch)
        # what the previous rollout prepared while its kernels ran (the same items, or it is not used)
        ahead, batch = self.__dict__.pop('_rollout_ahead', None), None
        if not (ahead is not None and ahead[0] is nav and len(ahead[1]) == len(items)
                and all(a is b for a, b in zip(ahead[1], items))):
            ahead = None
        if (self.test_graph and not reissue and not self.decoder.training and self.feedback == 'argmax'
                and self._engine.group is None):
            return self._rollout_on_graph(nav, items, ahead[2] if ahead is not None and isinstance(ahead[2], dict) else None)
        if ahead is not None and isinstance(ahead[2], DeviceNavBatch) and ahead[2].steps == self.episode_len:
            batch = ahead[2]
        if batch is None:
            batch = DeviceNavBatch(nav, items, self.episode_len, max_length=self.max_instruction_length,
                                   reverse=self.reverse_instruction)

        def prepare_next():
            # the minibatch the next env.reset will draw (peeked, not drawn: nothing changes if nobody comes for it):
            # encoded and packed on the host while this rollout's kernels run; its device tensors are filled behind them
            peek = getattr(self.env, 'peek_next_minibatch', None)
            nxt = peek(True) if peek is not None and self.prepare_ahead else None
            if nxt is not None:
                self._rollout_ahead = (nav, nxt, DeviceNavBatch(nav, nxt, self.episode_len,
                                                                max_length=self.max_instruction_length,
                                                                reverse=self.reverse_instruction))
        with per_step_kernels(self.encoder if reissue else None):
            st = self._engine.run(batch, self.episode_len, self.feedback, train=self.decoder.training,
                                  while_running=None if reissue else prepare_next)
        self.loss = st.loss
        traj = batch.trajectories(st)                   # the one host sync of the rollout
        for tr, it in zip(traj, items):
            tr['instr_encoding'] = it['instr_encoding']
        self.losses.append(float(st.loss.detach()))
        return traj

    test_graph = True            # argmax inference rollouts on the device environment: one hipGraph replay per minibatch

    def _test_graph_key(self, nav, eng, n_items):
        """What tells the captured inference rollouts of `_rollout_on_graph` apart (a capture keeps its gate-product mode)."""
        from .runtime import gate_mode_key
        return (id(nav), id(eng), self.episode_len, n_items, self.max_instruction_length,
                self.reverse_instruction) + gate_mode_key(eng.gate_weights)

    def _capture_test_rollout(self, nav, items, key, host=None):
        """Captures the inference rollout of `key` over a fixed-shape batch holding `items` and keeps it (at most three
        captures are kept): (replay, state, batch, nav, pinned result buffers)."""
        from .nav import DeviceNavBatch
        graphs = self.__dict__.setdefault('_test_graphs', {})
        S = self.episode_len
        batch = DeviceNavBatch(nav, items, S, max_length=self.max_instruction_length,
                               reverse=self.reverse_instruction, fixed_shapes=True, host=host)
        replay, st = self._engine.capture(batch, S, 'argmax')
        pinned = [torch.empty(t.shape, dtype=t.dtype).pin_memory()
                  for t in (batch.row[:S + 1], batch.view[:S + 1], st.actions, st.step_scores, st.loss_buf)]
        while len(graphs) >= 3:
            graphs.pop(next(iter(graphs)))
        graphs[key] = (replay, st, batch, nav, pinned)  # (nav kept alive: the key holds its id)
        return graphs[key]

    def _rollout_on_graph(self, nav, items, host=None):
        """An inference rollout (agent.test, follower.py:987-999) as ONE graph replay over a fixed-shape minibatch: the
        items are written into the captured batch's tensors (one pinned copy), the next minibatch is peeked and encoded
        while the replay runs, the fault word is read where the results are.  The results (and the fault words) come
        down asynchronously, and the NEXT minibatch's replay is issued right behind that download: the device runs it
        while the host builds this minibatch's dictionaries; the next call takes it over only for exactly the peeked
        items under exactly the current weight versions.  A starved persistent launch re-issues the minibatch on the
        per-step kernels (and drops what was issued ahead); weights that MOVED since the capture (load_state_dict into
        new tensors) mean a new capture.  Instructions are padded to max_instruction_length (the eager rollout pads to
        the minibatch's longest: equal up to the summation order of the padded attention columns).  `self.loss` is a
        host tensor on this path."""
        from .nav import DeviceNavBatch
        eng, dev = self._engine, self._device()
        key = self._test_graph_key(nav, eng, len(items))
        graphs = self.__dict__.setdefault('_test_graphs', {})  # (train.py alternates between its validation environments)
        S = self.episode_len
        # (key, items, weight versions): the replay the previous call issued ahead -- good for exactly these items under
        # exactly these weights
        versions = tuple((p_.data_ptr(), p_._version) for m in (self.encoder, self.decoder) for p_ in m.parameters())
        flying = self.__dict__.pop('_rollout_inflight', None)
        hit = (flying is not None and flying[0] == key and key in graphs and flying[2] == versions
               and len(flying[1]) == len(items) and all(a is b for a, b in zip(flying[1], items)))
        if hit:
            replay, st, batch, _, pinned = graphs[key]         # already loaded and replayed: its results wait on the device
        for attempt in () if hit else (0, 1):
            cached = graphs.get(key)
            if cached is None:
                replay, st, batch, _, pinned = self._capture_test_rollout(nav, items, key, host)
            else:
                replay, st, batch, _, pinned = cached
                batch.load(items, host)
            take_fault(dev)                                   # (whatever an earlier pass left behind is not ours)
            try:
                replay()
                break
            except WeightsMoved:                              # (only this: a device error is not a reason to recapture)
                if attempt:
                    raise
                graphs.pop(key, None)                         # a weight moved: capture again
        # this minibatch's results leave the device buffers before anything else is written into them ...
        for dst, src in zip(pinned, (batch.row[:S + 1], batch.view[:S + 1], st.actions, st.step_scores, st.loss_buf)):
            dst.copy_(src, non_blocking=True)
        # (the fault words travel with them: runtime.take_fault's synchronous copy would wait for the replay issued below)
        faults = fault_views(dev)
        fpin = self.__dict__.get('_fault_pin')
        if fpin is None or fpin.numel() != len(faults):
            fpin = self._fault_pin = torch.empty(len(faults), dtype=torch.int32).pin_memory()
        fpin.copy_(torch.cat(faults) if len(faults) > 1 else faults[0], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        # ... and the NEXT minibatch (peeked, not drawn) is encoded, loaded and replayed right behind them: the device
        # runs it while the host builds this minibatch's dictionaries
        peek = getattr(self.env, 'peek_next_minibatch', None)
        nxt = peek(True) if peek is not None and self.prepare_ahead else None
        if nxt is not None and len(nxt) == len(items):
            nhost = DeviceNavBatch.host_arrays_for(nav, nxt, self.max_instruction_length, self.reverse_instruction, True)
            try:
                batch.load(nxt, nhost)
                replay()
                self._rollout_inflight = (key, nxt, versions)
            except WeightsMoved:
                self._rollout_ahead = (nav, nxt, nhost)
        done.synchronize()
        rows, views, acts, sc, loss = (p_.numpy().copy() for p_ in pinned)
        if any(fpin.tolist()):
            self.__dict__.pop('_rollout_inflight', None)      # (what was issued ahead is not trusted either: reloaded next)
            torch.cuda.synchronize(dev)
            bits = take_fault(dev)                            # (read and cleared)
            batch.load(items)

            def eagerly():
                with torch.no_grad():
                    return eng.rollout(batch, S, 'argmax', train=False)
            st2 = reissue_per_step(self.encoder, eng, dev, 'an inference rollout', eagerly, bits)
            rows, views = batch.row[:S + 1].cpu().numpy(), batch.view[:S + 1].cpu().numpy()
            acts, sc, loss = st2.actions.cpu().numpy(), st2.step_scores.cpu().numpy(), st2.loss_buf.cpu().numpy()
        self.loss = torch.tensor(float(loss.reshape(-1)[0]))        # (a host tensor: a copy to the device would queue behind the replay issued ahead)
        traj = batch.trajectories_from(items, S, rows, views, acts, sc)
        for tr, it in zip(traj, items):
            tr['instr_encoding'] = it['instr_encoding']
        self.losses.append(float(loss.reshape(-1)[0]))
        return traj

    # ---- tensor assembly (follower.py:291-332): numpy stacks -> device tensors
    def _device(self):
        return next(self.decoder.parameters()).device

    def _feature_variables(self, obs):
        feats = np.stack([ob['feature'][0] for ob in obs])
        return [torch.from_numpy(feats).to(self._device())]

    def _action_variable(self, obs):
        max_a = max(len(ob['adj_loc_list']) for ob in obs)
        dim = obs[0]['action_embedding'].shape[-1]
        is_valid = np.zeros((len(obs), max_a), np.float32)
        emb = np.zeros((len(obs), max_a, dim), np.float32)
        for i, ob in enumerate(obs):
            n = len(ob['adj_loc_list'])
            is_valid[i, :n] = 1.0
            emb[i, :n] = ob['action_embedding']
        dev = self._device()
        return torch.from_numpy(emb).to(dev), torch.from_numpy(is_valid).to(dev), is_valid

    def _teacher_action(self, obs, ended):
        a = torch.tensor([ob['teacher'] if not ended[i] else -1 for i, ob in enumerate(obs)],
                         dtype=torch.int64)
        return a.to(self._device())

    def _proc_batch(self, obs):
        enc = [ob['instr_encoding'] for ob in obs]
        return batch_instructions_from_encoded(enc, self.max_instruction_length,
                                               reverse=self.reverse_instruction,
                                               device=self._device())

    def rollout(self):
        if self.beam_size == 1:                                        # follower.py:334-340
            return self._rollout_with_loss()
        assert self.beam_size >= 1
        beams, _, _ = self.beam_search(self.beam_size)
        return [beam[0] for beam in beams]

    # beam_search with its step loop on the device (search.DeviceFollowerBeam: no host round trip per decode step, chunks
    # of `beam_chunk` steps as replayed hipGraphs, or issued eagerly with beam_graphs = False).  Off by default.  Same
    # results as the host loop up to the roundoff of a decoder step over other row counts; inference only;
    # beam_size <= 64 -- wider beams run the host loop and count a fallback.
    beam_on_device = False
    beam_chunk = 2
    beam_graphs = True
    beam_fallbacks = 0
    device_beam = None

    def beam_search(self, beam_size, load_next_minibatch=True, mask_undo=False):
        """follower.py:541-718 (search.py; needs `self.store` and index-form observations)."""
        from . import search
        return search.beam_search(self, beam_size, load_next_minibatch, mask_undo)

    # state_factored_search with its iteration loop on the device (search.DeviceStateFactored: the bookkeeping of
    # sim/frontier_core.cpp in sf_state_factored_select, chunks of `search_chunk` iterations as replayed hipGraphs -- or
    # issued eagerly with search_graphs = False --, one small status read per chunk).  Off by default.  Same results as the host loop, bit for bit (the decoder step sees
    # the same rows in the same positions); inference only.  search_backend = 'numpy', a tie_log, a decoder without the
    # visual attention, a shape beyond the kernel (search.DeviceStateFactored.supports) or a search that overflows
    # `search_node_cap` nodes / `search_slot_cap` dictionary entries per instance runs the host loop from its start and
    # counts a fallback.
    search_on_device = False
    search_chunk = 4
    search_graphs = True
    search_node_cap = 2048
    search_slot_cap = 1024
    search_fallbacks = 0
    device_search = None

    def state_factored_search(self, completion_size, successor_size, load_next_minibatch=True,
                              mask_undo=False, first_n_ws_key=4):
        """follower.py:720-980."""
        from . import search
        return search.state_factored_search(self, completion_size, successor_size,
                                            load_next_minibatch, mask_undo, first_n_ws_key)

    def set_beam_size(self, beam_size):
        if getattr(self.env, 'beam_size', 1) < beam_size:
            self.env.set_beam_size(beam_size)
        self.beam_size = beam_size

    def _step(self, u_prev, obs, h, c, ctx, seq_mask, target, feedback, ended_dev):
        """One decoder step + glue on dense observations (follower.py:469-505)."""
        f_t = self._feature_variables(obs)[0]
        all_u, is_valid, _ = self._action_variable(obs)
        h, c, alpha, logit, alpha_v = self.decoder(u_prev, all_u, f_t, h, c, ctx, seq_mask)
        self._sample_count += 1
        ce, live, a_t, score, u_next, masked = _FollowerGlueFn.apply(
            logit, all_u, is_valid, target, FEEDBACK[feedback], ended_dev,
            (self._sample_seed, self._sample_count))
        n_live = live.sum()
        loss_t = ce.sum() / n_live.clamp(min=1.0)                    # CrossEntropyLoss mean over live
        return h, c, loss_t, a_t, score, u_next

    def _rollout_with_loss(self, reissue=False):
        """follower.py:430-539."""
        table = self._device_table()
        if table is not None:
            return self._rollout_on_device(table, reissue)
        world_states = self.env.reset(sort=True)
        obs = np.array(self.env.observe(world_states))
        B = len(obs)
        seq, seq_mask, seq_lengths = self._proc_batch(obs)
        self.loss = 0
        feedback = self.feedback
        ctx, h, c = self.encoder(seq, seq_lengths)
        traj = [{'instr_id': ob['instr_id'], 'trajectory': [path_element_from_observation(ob)],
                 'actions': [], 'scores': [], 'observations': [ob],
                 'instr_encoding': ob['instr_encoding']} for ob in obs]
        dev = self._device()
        u_prev = self.decoder.u_begin.to(dev).expand(B, -1).contiguous()
        ended = np.array([False] * B)
        ended_dev = torch.zeros(B, dtype=torch.uint8, device=dev)
        seq_scores = torch.zeros(B, device=dev)
        for t in range(self.episode_len):
            target = self._teacher_action(obs, ended)
            ended_dev.zero_()      # `target` already carries -1 for ended rows (follower.py:327)
            h, c, loss_t, a_t, score, u_prev = self._step(u_prev, obs, h, c, ctx, seq_mask, target,
                                                          feedback, ended_dev)
            self.loss = self.loss + loss_t
            seq_scores = seq_scores + score
            actions = a_t.tolist()                                     # the per-step D2H sync (:509-511)
            world_states = self.env.step(world_states, actions, obs)
            obs = self.env.observe(world_states)
            sc, ss = score.tolist(), seq_scores.tolist()
            for i, ob in enumerate(obs):
                if not ended[i]:
                    traj[i]['trajectory'].append(path_element_from_observation(ob))
                    traj[i]['score'] = ss[i]
                    traj[i]['scores'].append(sc[i])
                    traj[i]['actions'].append(actions[i])
                    traj[i]['observations'].append(ob)
            for i in range(B):
                if actions[i] == 0:
                    ended[i] = True
            if ended.all():
                break
        self.losses.append(float(self.loss.detach()) if torch.is_tensor(self.loss) else float(self.loss))
        return traj

    SCORE_CHUNK = 256          # rows of one teacher-forced pass of an index-form scoring call (inference)
    score_on_device = False    # True: observations with dense features are scored through the device pass as well

    def _score_obs_actions_and_instructions(self, path_obs, path_actions, encoded_instructions):
        """follower.py:342-428: teacher-forced scoring of given paths.  Observations in index form (no 'feature' /
        'action_embedding': an env that carries its feature store), or any with `score_on_device`, go through
        _score_routes_on_device; dense ones through the per-step host loop below."""
        B = len(path_obs)
        assert len(path_actions) == B and len(encoded_instructions) == B
        if self.score_on_device or 'feature' not in path_obs[0][0]:
            store = self.store if self.store is not None else self._env_store()
            if store is None:
                raise RuntimeError('index-form observations need a features.FeatureStore (agent.store or '
                                   'env.image_features_list[0].store)')
            return self._score_routes_on_device(path_obs, path_actions, encoded_instructions, store)
        dev = self._device()
        seq, seq_mask, seq_lengths, perm = batch_instructions_from_encoded(
            encoded_instructions, self.max_instruction_length, reverse=self.reverse_instruction,
            sort=True, device=dev)
        loss = 0
        ctx, h, c = self.encoder(seq, seq_lengths)
        u_prev = self.decoder.u_begin.to(dev).expand(B, -1).contiguous()
        ended = np.array([False] * B)
        ended_dev = torch.zeros(B, dtype=torch.uint8, device=dev)
        seq_scores = torch.zeros(B, device=dev)
        traj = [{'instr_id': po[0]['instr_id'], 'trajectory': [path_element_from_observation(po[0])],
                 'actions': [], 'scores': [], 'observations': [po[0]],
                 'instr_encoding': po[0]['instr_encoding']} for po in path_obs]
        obs = None
        for t in range(self.episode_len):
            nxt, tgt = [], []
            for pi, si in enumerate(perm):
                if t < len(path_actions[si]):
                    tgt.append(path_actions[si][t])
                    nxt.append(path_obs[si][t])
                else:
                    tgt.append(-1)
                    nxt.append(obs[pi])
            obs = nxt
            target = torch.tensor(tgt, dtype=torch.int64, device=dev)
            h, c, loss_t, a_t, score, u_prev = self._step(u_prev, obs, h, c, ctx, seq_mask, target,
                                                          'teacher', ended_dev)
            ended_dev.zero_()
            loss = loss + loss_t
            live = (target != -1).to(score.dtype)
            seq_scores = seq_scores + score * live                     # :405 ignore_index rows score 0
            acts, sc, ss = a_t.tolist(), (score * live).tolist(), seq_scores.tolist()
            for pi, si in enumerate(perm):
                if not ended[pi]:
                    traj[si]['trajectory'].append(path_element_from_observation(obs[pi]))
                    traj[si]['score'] = ss[pi]
                    traj[si]['scores'].append(sc[pi])
                    traj[si]['actions'].append(acts[pi])
            for i in range(B):
                if acts[i] == 0:
                    ended[i] = True
            if ended.all():
                break
        return traj, loss

    def _scoring_engine(self, store):
        from .follower import FollowerEngine
        eng = self.__dict__.get('_score_engine')
        if eng is None or eng.store is not store or eng.encoder is not self.encoder or eng.decoder is not self.decoder:
            eng = self._score_engine = FollowerEngine(self.encoder, self.decoder, store)
            eng.dropout_seed = self._sample_seed ^ 0x1B873593
            eng.gate_weights = self.gate_weights
        return eng

    @gc_paused
    def _score_routes_on_device(self, path_obs, path_actions, encoded_instructions, store):
        """The same scoring as teacher-forced FollowerEngine passes over the routes in index form
        (follower.route_index_batch).  Inference walks the rows in chunks of SCORE_CHUNK, in the caller's order, each
        chunk over its own steps; every chunk is uploaded before the first is issued, so nothing waits for the device
        until the ONE download of the actions, step scores, live flags, loss and fault words at the end.  The loss
        (per step, the mean over the live rows of ALL chunks) is re-assembled from the chunks' (sum, count) tables.  With
        autograd on, or in train mode, one unchunked pass whose loss backpropagates through the engine's backward.  A
        starved persistent encoder launch re-issues the whole call on the per-step kernels (FollowerEngine.run).
        `last_host_reads` counts the host synchronisations of the call."""
        from .follower import DeviceFollowerBatch, route_index_batch, scored_route_outputs
        B = len(path_obs)
        eng, dev = self._scoring_engine(store), store.device
        training = self.decoder.training
        step = B if (training or torch.is_grad_enabled()) else self.SCORE_CHUNK
        chunks = []
        for lo in range(0, B, step):
            hi = min(lo + step, B)
            fb, S_k = route_index_batch(path_obs[lo:hi], path_actions[lo:hi], encoded_instructions[lo:hi], self.episode_len)
            chunks.append((lo, hi, S_k, DeviceFollowerBatch.from_synth(fb, device=dev, max_length=self.max_instruction_length,
                                                                       reverse=self.reverse_instruction, row0=lo)))
        S = max(c[2] for c in chunks)

        def issue():
            out = torch.zeros(3, S, B, device=dev)                 # actions, step scores, live
            total, last = None, None
            for lo, hi, S_k, batch in chunks:
                st = eng.rollout(batch, S_k, 'teacher', train=training, finalize=False)
                out[0, :S_k, lo:hi] = st.actions
                out[1, :S_k, lo:hi] = st.step_scores
                out[2, :S_k, lo:hi] = st.live
                if len(chunks) > 1:
                    if total is None:
                        total = torch.zeros(S, 2, device=dev)
                    total[:S_k] += st.sum_cnt
                if S_k == S and last is None:
                    last = st
            eng.finish(last, total)
            faults = fault_views(dev)
            flat = torch.cat([out.reshape(-1), last.loss_buf] + [f.to(torch.float32) for f in faults])
            return last, flat.cpu()                                 # (the one host sync)

        site, it = eng.site_next, eng.iteration
        st, flat = issue()
        reads = 1
        raised = [int(w) for w in flat[3 * S * B + 1:].tolist() if w]
        if raised:
            for w in fault_views(dev):                              # (read with the results: cleared here)
                w.zero_()
            eng.site_next, eng.iteration = site, it
            st, flat = reissue_per_step(self.encoder, eng, dev, 'a route scoring pass', issue, int(np.bitwise_or.reduce(raised)))
            reads += 2                                              # (its download, and the helper's look at the fault words)
        self.last_host_reads = reads
        res = flat[:3 * S * B].numpy().reshape(3, S, B)
        traj = scored_route_outputs(path_obs, path_actions, res[0], res[1], res[2])
        return traj, st.loss

    def test(self, use_dropout=False, feedback='argmax', allow_cheat=False, beam_size=1):
        """follower.py:987-999."""
        if not allow_cheat:
            assert feedback in ['argmax', 'sample']
        self.feedback = feedback
        for m in (self.encoder, self.decoder):
            m.train() if use_dropout else m.eval()
        self.set_beam_size(beam_size)
        self.__dict__.pop('_rollout_inflight', None)          # (nothing issued ahead by an earlier loop is ours)
        # (test() reads results, nothing differentiates them: without autograd a rollout keeps no tape -- a differentiable
        # state lives until the cyclic collector finds it, a few hundred MB per minibatch)
        with torch.no_grad():
            return super().test()

    def train(self, encoder_optimizer, decoder_optimizer, n_iters, feedback='teacher'):
        """follower.py:1001-1020."""
        assert all(f in self.feedback_options for f in feedback.split('+'))
        self.feedback = feedback
        self.encoder.train()
        self.decoder.train()
        self.losses = []
        if self._graph_trainable(encoder_optimizer, decoder_optimizer):
            return self._train_on_graph(encoder_optimizer, decoder_optimizer, n_iters)
        for _ in range(1, n_iters + 1):
            encoder_optimizer.zero_grad()
            decoder_optimizer.zero_grad()
            eng = self._engine if self._device_table() is not None else None
            where = (eng.site_next, eng.iteration) if eng is not None else None
            self._rollout_with_loss()
            self.loss.backward()
            # a starved persistent launch of the BACKWARD has poisoned the gradients: never step on them -- replay
            # the minibatch on the per-step kernels (the forward's own check sits inside FollowerEngine.run)
            bits = fault_bits(self._device())
            if bits:
                encoder_optimizer.zero_grad()
                decoder_optimizer.zero_grad()
                self.losses.pop()
                if where is not None:
                    eng.site_next, eng.iteration = where       # (the masks / samples the poisoned rollout drew)

                def again():
                    # (the device environment replays the SAME minibatch; the per-step host loop cannot rewind its
                    # simulators and trains on the next one)
                    self._rollout_with_loss(reissue=True)
                    self.loss.backward()
                reissue_per_step(self.encoder, eng, self._device(), 'a training iteration', again, bits)
            encoder_optimizer.step()
            decoder_optimizer.step()

    # ---- training iterations as hipGraph replays (runtime.TrainingGraph) ------------------------------------------
    train_graph = True           # False: every iteration issued launch by launch (the loop above)

    def _graph_trainable(self, encoder_optimizer, decoder_optimizer):
        """Whole iterations can be replayed when the environment is walked on the device, both optimizers keep their
        state in flat buffers with device-side step counters (optim.FusedAdam) and nothing leaves the process."""
        return self._why_not_graph_trainable(encoder_optimizer, decoder_optimizer) is None

    def _why_not_graph_trainable(self, encoder_optimizer, decoder_optimizer):
        """None where `_graph_trainable` holds, else the first condition that fails, in words."""
        from .optim import FusedAdam
        if not self.train_graph:
            return 'train_graph is off'
        if '+' in self.feedback:
            return "'+' feedback"
        if self.beam_size != 1:
            return 'a beam'
        for o in (encoder_optimizer, decoder_optimizer):
            if not (isinstance(o, FusedAdam) or (self.adopt_torch_adam and FusedAdam.adoptable(o))):
                return 'an optimizer that is neither an optim.FusedAdam nor a torch Adam it can adopt'
        if self._device_table() is None or self._engine is None:
            return 'no navigation table on the device'
        eng = self._engine
        alone = eng.group is None and eng.grad_sync is None
        # (a process group: iterations replay as SEGMENTS cut at the collective points, FollowerEngine._capture_training_dp;
        # that needs the gradient buckets the all-reduces work on)
        if not (alone or (eng.group is not None and eng.grad_sync is not None)):
            return 'a process group without its gradient buckets'
        # (a bidirectional encoder: single process only -- its data-parallel iteration keeps the eager loop)
        if getattr(self.encoder, 'num_directions', 1) != 1 and not alone:
            return 'a bidirectional encoder under a process group'
        if not getattr(self.encoder, 'persistent', True):
            return 'an encoder without its persistent launch'
        return None

    def _train_on_graph(self, encoder_optimizer, decoder_optimizer, n_iters):
        """follower.py:1001-1020 with every iteration after the first ONE graph replay: the next minibatch is written
        into the captured batch's tensors (nav.DeviceNavBatch.load), dropout sites / samples / Adam steps advance
        through device words, and the optimizer steps are GUARDED by the fault word of the persistent launches
        (sf_adam_step_dev: a starved launch turns them into no-ops) -- the host looks at the word where it reads the
        loss and re-issues that iteration on the per-step kernels.  Same sites, same numbers as the eager loop
        (tests/test_gpu_agents.py)."""
        from .nav import DeviceNavBatch
        table, eng, dev = self._device_table(), self._engine, self._device()
        given = (encoder_optimizer, decoder_optimizer)
        opts = tuple(self._fused_for(o) for o in given)
        try:
            return self._replay_iterations(opts, n_iters, table, eng, dev)
        finally:
            for o, f in zip(given, opts):             # the reference's own optimizer objects get their state back
                if f is not o:
                    f.store_torch_state(o)

    prepare_ahead = True         # train() on graphs: the next minibatch's host work under the current replay
    adopt_torch_adam = True      # train(): a plain torch.optim.Adam (train.py:263-268) is mirrored by an optim.FusedAdam

    def _fused_for(self, opt):
        """`opt` itself (optim.FusedAdam), or the FusedAdam that mirrors this torch.optim.Adam: same parameters (their
        data moves into one flat buffer, once), hyper-parameters and state taken over at the start of every train() call
        and handed back at its end -- checkpoints of `opt.state_dict()` and steps taken elsewhere stay consistent."""
        import weakref
        from .optim import FusedAdam
        if isinstance(opt, FusedAdam):
            return opt
        mirrors = self.__dict__.setdefault('_fused_mirrors', {})
        hit = mirrors.get(id(opt))
        if hit is None or hit[0]() is not opt:
            g = opt.param_groups[0]
            fused = FusedAdam(g['params'], lr=g['lr'], betas=tuple(g['betas']), eps=g['eps'], weight_decay=g['weight_decay'])
            mirrors[id(opt)] = hit = (weakref.ref(opt), fused)
        hit[1].load_torch_state(opt)
        return hit[1]

    def _train_graph_key(self, opts, table):
        """What tells the captured training iterations apart (a captured iteration holds the optimizers'
        hyper-parameters as kernel arguments: a changed learning rate is a new graph)."""
        hyper = tuple((g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) for o in opts for g in o.param_groups)
        return (id(opts[0]), id(opts[1]), self.feedback, id(table), self.episode_len, hyper)

    def _train_pins_for(self, n_words):
        """Two pinned (loss, fault words) pairs for the pipelined replays (one fault word per workspace; a workspace
        created later -- a side stream of the per-step fallback -- makes the list longer: the pairs are re-made to match)."""
        pins = self.__dict__.get('_train_pins')
        if pins is None or pins[0][1].numel() != n_words:
            pins = self._train_pins = [(torch.empty(1, dtype=torch.float32).pin_memory(),
                                        torch.empty(n_words, dtype=torch.int32).pin_memory()) for _ in range(2)]
        return pins

    def train_on_routes(self, routes, encoder_optimizer, decoder_optimizer, n_iters, feedback='teacher', batch_size=100,
                        order=None, seed=0):
        """`train` over a routes.RouteSet instead of the environment (train.py --use_pretraining on an augmentation
        split, with no file and no environment object in between): the same replayed iterations, their minibatches
        drawn from `routes.pack_follower(batch_size, ...)` -- packed on the device by sf_nav_follower_batches, ONE
        device-to-device copy per iteration (nav.DeviceNavBatch.load_packed).  order: the route index of every slot,
        n_iters * batch_size of them (default `routes.epoch_order(batch_size, n_iters, seed)`); a minibatch is sorted by
        instruction length as env.reset(sort=True) sorts it.  The captured graph is `train`'s own where optimizers,
        feedback, table and batch size match.  The minibatches are packed `route_window` (default routes.PACK_CHUNK = 256)
        at a time, one launch and one host sync per window, at most two windows alive: 2 x 256 x 213 KB at B = 100, 80
        words, however long the call.  Only what can be replayed in ONE process is supported: NotImplementedError names
        what stands in the way (a process group among them: data-parallel training on routes is not built)."""
        assert all(f in self.feedback_options for f in feedback.split('+'))
        self.feedback = feedback
        self.encoder.train()
        self.decoder.train()
        self.losses = []
        # (data-parallel training on routes is not built: the pipelined loop below decides about a fault from this
        # process's own words, and every rank would draw the same order -- refused whatever else holds)
        why = self._why_not_graph_trainable(encoder_optimizer, decoder_optimizer)
        eng = self._engine
        if eng is not None and (eng.group is not None or eng.grad_sync is not None):
            why = 'a process group'
        if why is not None:
            raise NotImplementedError('train_on_routes replays captured iterations in one process only: ' + why)
        table, eng, dev = self._device_table(), self._engine, self._device()
        if routes.nav is not table:
            raise ValueError("train_on_routes: the routes' navigation table is not the agent's device table")
        B = int(batch_size)
        if order is None:
            order = routes.epoch_order(B, n_iters, seed)
        order = np.ascontiguousarray(order, np.int32).reshape(-1)
        if len(order) != n_iters * B:
            raise ValueError('train_on_routes: an order of %d slots for %d iterations of %d' % (len(order), n_iters, B))
        if n_iters < 1:
            return
        # (packed a window of minibatches at a time: the blocks of a whole call would be n_iters x 213 KB at B = 100)
        blocks = routes.follower_windows(B, self.max_instruction_length, order, reverse=self.reverse_instruction,
                                         window=self.route_window)
        given = (encoder_optimizer, decoder_optimizer)
        opts = tuple(self._fused_for(o) for o in given)
        try:
            return self._replay_route_blocks(opts, n_iters, routes, order, blocks, table, eng, dev)
        finally:
            for o, f in zip(given, opts):             # the reference's own optimizer objects get their state back
                if f is not o:
                    f.store_torch_state(o)

    route_window = None          # train_on_routes: minibatches packed per pack_follower call (None: routes.PACK_CHUNK)

    def _replay_route_blocks(self, opts, n_iters, routes, order, blocks, table, eng, dev):
        """`_replay_iterations` / `_replay_pipelined` over routes.FollowerWindows: iteration i is load_packed(*blocks.at(i))
        and a replay, replay i + 1 queued before the loss of replay i is read.  Where no graph exists yet, iteration 0
        captures it over a batch built from the host form of the same minibatch (RouteSet.follower_minibatch_host)."""
        from .nav import DeviceNavBatch
        key = self._train_graph_key(opts, table)
        cached = self.__dict__.get('_train_graph_state')
        take_fault(dev)                                       # (whatever an earlier pass left behind is not ours)
        if cached is not None and (cached[0] != key or cached[2].batch_size != blocks.B):
            cached = None
        issued = 0
        if cached is None:
            before = [o.host_steps() for o in opts]
            where = (eng.site_next, eng.iteration)
            host = routes.follower_minibatch_host(order[:blocks.B], blocks.Lmax, reverse=self.reverse_instruction)
            batch = DeviceNavBatch(table, host['route'].tolist(), self.episode_len, max_length=self.max_instruction_length,
                                   reverse=self.reverse_instruction, fixed_shapes=True, host=host)
            for o in opts:
                o.guard_faults = True
            tg = eng.capture_training(batch, self.episode_len, self.feedback, optimizers=opts, zero=eng.grad_sync)
            cached = self._train_graph_state = (key, tg, batch)
            st = tg.first                                     # (the capture ran this iteration eagerly)
            loss = float(st.loss_buf)
            bits = fault_bits(dev, eng.group)
            if bits:
                batch.load_packed(*blocks.at(0))
                st = self._reissue_training_iteration(opts, eng, dev, batch, before, where, bits)
                loss = float(st.loss_buf)
            self.loss = st.loss_buf.reshape(())
            self.losses.append(loss)
            issued = 1
            if n_iters == 1:
                return
        _, tg, batch = cached
        flight = None                  # the iteration whose loss has not been read: (slot, event, state before it, block, pins)
        while issued < n_iters or flight is not None:
            cur = None
            if issued < n_iters:
                before = ([o.host_steps() for o in opts], eng.site_next, eng.iteration)
                batch.load_packed(*blocks.at(issued))
                st = tg.replay()
                slot = issued & 1
                views = fault_views(dev)
                if flight is not None and flight[4][0][1].numel() != len(views):
                    flight[1].synchronize()                   # (the pair in flight is read before it is replaced)
                pins = self._train_pins_for(len(views))
                pins[slot][0].copy_(st.loss_buf.reshape(1), non_blocking=True)
                pins[slot][1].copy_(torch.cat(views) if len(views) > 1 else views[0], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                cur = (slot, ev, before, issued, pins)
                issued += 1
            if flight is not None:
                slot, ev, before_f, block_f, pins = flight
                ev.synchronize()
                if any(pins[slot][1].tolist()):
                    torch.cuda.synchronize(dev)               # (the replay queued behind it did nothing either)
                    bits = take_fault(dev)
                    batch.load_packed(*blocks.at(block_f))
                    st2 = self._reissue_training_iteration(opts, eng, dev, batch, before_f[0], before_f[1:], bits)
                    self.losses.append(float(st2.loss_buf))
                    if cur is not None:                       # the one queued behind it is issued again
                        issued -= 1
                        cur = None
                else:
                    self.losses.append(float(pins[slot][0]))
            flight = cur
        self.loss = tg.state.loss_buf.reshape(())

    def _replay_iterations(self, opts, n_iters, table, eng, dev):
        from .nav import DeviceNavBatch
        key = self._train_graph_key(opts, table)
        cached = self.__dict__.get('_train_graph_state')
        take_fault(dev)                                       # (whatever an earlier pass left behind is not ours)
        ahead = None            # the NEXT minibatch and its host arrays, formed while the device ran this iteration
        for it in range(n_iters):
            if (self.pipeline_replays and self.prepare_ahead and cached is not None and cached[0] == key
                    and cached[2].batch_size == self.env.batch_size and eng.group is None):
                # the graph exists: the remaining iterations with one replay always queued behind the running one
                return self._replay_pipelined(opts, n_iters - it, cached, eng, dev, ahead)
            if ahead is None:
                self.env.reset(sort=True)
                items, host = list(self.env.batch), None
            else:
                items, host = ahead
                ahead = None
            before = [o.host_steps() for o in opts]
            where = (eng.site_next, eng.iteration)            # the dropout / sample sites this iteration starts at
            if cached is not None and (cached[0] != key or cached[2].batch_size != len(items)):
                cached = None
            if cached is None:
                batch = DeviceNavBatch(table, items, self.episode_len, max_length=self.max_instruction_length,
                                       reverse=self.reverse_instruction, fixed_shapes=True)
                for o in opts:
                    o.guard_faults = True
                tg = eng.capture_training(batch, self.episode_len, self.feedback, optimizers=opts, zero=eng.grad_sync)
                cached = self._train_graph_state = (key, tg, batch)
                st = tg.first                                 # (the capture ran this iteration eagerly)
            else:
                _, tg, batch = cached
                batch.load(items, host)
                st = tg.replay()
            if self.prepare_ahead and it + 1 < n_iters:
                # the replay is in flight: draw the next minibatch (the same env.reset calls in the same order, earlier)
                # and encode it now; its copies wait until this iteration's loss has been read
                self.env.reset(sort=True)
                nxt = list(self.env.batch)
                ahead = (nxt, batch._host_arrays(nxt) if len(nxt) == batch.batch_size else None)
            loss = float(st.loss_buf)                         # the iteration's one host sync
            bits = fault_bits(dev, eng.group)                 # (every rank takes the same decision)
            if bits:
                # a persistent launch starved: the guarded optimizer steps did nothing.  The same minibatch again on
                # the per-step kernels, launch by launch
                if eng.grad_sync is not None:
                    eng.grad_sync.abort()                     # (nothing of the faulted round is in flight: replays wait)
                st = self._reissue_training_iteration(opts, eng, dev, batch, before, where, bits)
                loss = float(st.loss_buf)
            self.loss = st.loss_buf.reshape(())
            self.losses.append(loss)

    def _reissue_training_iteration(self, opts, eng, dev, batch, steps_before, where, bits):
        """A replayed training iteration whose persistent launch raised fault `bits` (its guarded optimizer steps did
        nothing), again on the per-step kernels, launch by launch: the optimizers' host steps and the dropout / sampling
        sites (`where`) as they were in front of the replay, so that it draws the masks and samples the replay drew, over
        what `batch` holds.  Steps the optimizers and returns the rollout's state (runtime.reissue_per_step)."""
        for o, b in zip(opts, steps_before):
            o.set_host_steps(b)
            o.zero_grad()
        eng.site_next, eng.iteration = where

        def launch_by_launch():
            st = eng.rollout(batch, self.episode_len, self.feedback, train=True)
            st.loss.backward()
            if eng.grad_sync is not None:
                eng.grad_sync.wait()
            return st
        st = reissue_per_step(self.encoder, eng, dev, 'a training iteration', launch_by_launch, bits)
        for o in opts:
            o.step()
        return st

    pipeline_replays = True      # train() on graphs: replay i + 1 is queued before the loss of replay i is read

    def _replay_pipelined(self, opts, n, cached, eng, dev, first=None):
        """`n` iterations of `_replay_iterations` with the device never waiting for the host: replay i + 1 (its minibatch
        loaded behind replay i on the same stream) is queued BEFORE the host waits for iteration i, whose loss and fault
        words come down asynchronously into pinned memory.  Nothing on the device depends on the host reading a loss;
        the one thing that does is the fault path: the guarded optimizer steps of a faulted iteration AND of the one
        queued behind it do nothing (the fault word stays raised until the host clears it), so the host re-issues the
        faulted minibatch on the per-step kernels and queues the other one again.  Same minibatches in the same order,
        same sites, same steps: losses and weights of the serial loop (tests/test_gpu_nav.py)."""
        import collections
        _, tg, batch = cached
        pins_for = self._train_pins_for
        todo = collections.deque()     # minibatches drawn and not issued yet: (items, host arrays or None)
        drawn = issued = 0
        if first is not None:          # (what the serial loop had already drawn for its next iteration)
            todo.append(first)
            drawn = 1
        flight = None                  # the iteration whose loss has not been read: (slot, event, steps before it, items)

        def draw():
            nonlocal drawn
            self.env.reset(sort=True)
            nxt = list(self.env.batch)
            todo.append((nxt, batch._host_arrays(nxt) if len(nxt) == batch.batch_size else None))
            drawn += 1
        while issued < n or flight is not None:
            cur = None
            if issued < n:
                if not todo:
                    draw()
                items, host = todo.popleft()
                before = ([o.host_steps() for o in opts], eng.site_next, eng.iteration)
                batch.load(items, host)
                st = tg.replay()
                slot = issued & 1
                views = fault_views(dev)
                if flight is not None and flight[4][0][1].numel() != len(views):
                    flight[1].synchronize()                   # (the pair in flight is read before it is replaced)
                pins = pins_for(len(views))
                pins[slot][0].copy_(st.loss_buf.reshape(1), non_blocking=True)
                pins[slot][1].copy_(torch.cat(views) if len(views) > 1 else views[0], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                cur = (slot, ev, before, items, pins)
                issued += 1
            if flight is not None:
                slot, ev, before_f, items_f, pins = flight
                ev.synchronize()
                if any(pins[slot][1].tolist()):
                    torch.cuda.synchronize(dev)               # (the replay queued behind it did nothing either)
                    bits = take_fault(dev)
                    batch.load(items_f)
                    # (the sites of the faulted replay: it and the one queued behind it advanced the host mirrors)
                    st2 = self._reissue_training_iteration(opts, eng, dev, batch, before_f[0], before_f[1:], bits)
                    self.losses.append(float(st2.loss_buf))
                    if cur is not None:                       # queue the other one again, in front of what was drawn since
                        todo.appendleft((cur[3], None))
                        issued -= 1
                        cur = None
                else:
                    self.losses.append(float(pins[slot][0]))
            flight = cur
            if flight is not None and drawn < n and not todo:
                draw()                                        # (host work under the replay that is running)
        self.loss = tg.state.loss_buf.reshape(())

    def _encoder_and_decoder_paths(self, base_path):
        return base_path + '_enc', base_path + '_dec'

    def save(self, path):
        ep, dp = self._encoder_and_decoder_paths(path)
        torch.save(self.encoder.state_dict(), ep)
        torch.save(self.decoder.state_dict(), dp)

    def load(self, path, **kwargs):
        ep, dp = self._encoder_and_decoder_paths(path)
        self.encoder.load_state_dict(torch.load(ep, **kwargs))
        self.decoder.load_state_dict(torch.load(dp, **kwargs))


class _SpeakerGlueFn(torch.autograd.Function):
    """speaker.py:163-191 on a [B,vocab] logit tensor."""

    @staticmethod
    def forward(ctx, logit, target, feedback, ended_dev, pad_idx, eos_idx, sample_cfg=None):
        B, V = logit.shape
        ldv = (V + 3) & ~3
        dev = logit.device
        lg = torch.zeros(B, ldv, device=dev)
        lg[:, :V] = logit.detach()
        w_t = torch.empty(B, dtype=torch.int64, device=dev)
        score, nll, live = (torch.empty(B, device=dev) for _ in range(3))
        smp = byref(_lib.Sample(sample_cfg[0] & 0xFFFFFFFF, sample_cfg[1] & 0xFFFFFFFF, 0)) if feedback == 2 else None
        call('sf_speaker_glue_fwd', B, V, ldv, ptr(lg), ptr(target), feedback, pad_idx, eos_idx,
             ptr(ended_dev), ptr(w_t), ptr(score), ptr(nll), ptr(live), smp, stream())
        ctx.save_for_backward(lg, target)
        ctx.cfg = (B, V, ldv, pad_idx)
        ctx.mark_non_differentiable(live, w_t, score)
        return nll, live, w_t, score

    @staticmethod
    def backward(ctx, dnll, *_):
        lg, target = ctx.saved_tensors
        B, V, ldv, pad_idx = ctx.cfg
        one = torch.ones(1, device=lg.device)
        dl = torch.empty_like(lg)
        call('sf_speaker_glue_bwd', B, V, ldv, ptr(lg), ptr(target), pad_idx, ptr(one), ptr(dl),
             stream())
        return dl[:, :V] * dnll.reshape(B, 1), None, None, None, None, None, None


class _ScoredInstruction(LazyDict):
    """One output of Seq2SeqSpeaker._score_obs_actions_and_instructions (speaker.py:139-141, 198-202): 'instr_id' and
    'score' are there; 'word_indices', 'scores' and 'words' are cut from the batch's arrays when somebody reads them
    (the pragmatic re-ranking reads the score of 2 500 routes and nothing else, rational_follower.py:70-74)."""
    __slots__ = ('_w', '_s', '_m', '_tok')

    def __init__(self, instr_id, score, words_row, scores_row, m, tok):
        LazyDict.__init__(self, {'instr_id': instr_id, 'score': score}, ('word_indices', 'scores', 'words'))
        self._w, self._s, self._m, self._tok = words_row, scores_row, m, tok

    def _make(self, key):
        if key == 'scores':
            return self._s[:self._m].tolist()
        wi = self['word_indices'] if key == 'words' else self._w[:self._m].tolist()
        if key == 'words' and self._tok is not None:
            return self._tok.decode_sentence(wi, break_on_eos=True, join=False)
        return wi


class _PendingScores:
    """A chunked scoring sweep that has been issued and not collected yet (Seq2SeqSpeaker._issue_scores)."""
    obs_lists = None

    def matches(self, path_obs, feedback):
        return (self.obs_lists is not None and feedback == self.feedback and len(path_obs) == len(self.obs_lists)
                and all(a is b for a, b in zip(path_obs, self.obs_lists)))


def _ragged(counts):
    """[0..c0-1, 0..c1-1, ...] and the index of the owner of each element."""
    owner = np.repeat(np.arange(len(counts)), counts)
    starts = np.cumsum(counts) - counts
    return np.arange(len(owner)) - starts[owner], owner


class Seq2SeqSpeaker(object):
    """speaker.py:34-410 (teacher / argmax / sample decoding, scoring, train, save/load)."""
    feedback_options = ['teacher', 'argmax', 'sample']

    def __init__(self, env, results_path, encoder, decoder, instruction_len, max_episode_len=10):
        self.env = env
        self.results_path = results_path
        random.seed(1)
        self.results = {}
        self.losses = []
        self.encoder, self.decoder = encoder, decoder
        self.instruction_len = instruction_len
        self.max_episode_len = max_episode_len
        self.feedback = 'argmax'
        self._sample_seed = torch.initial_seed() & 0xFFFFFFFF     # `sample` feedback: counter-based draws (sf_sampling.h)
        self._sample_count = 0

    def write_results(self):
        with open(self.results_path, 'w') as f:
            json.dump(self.results, f)

    def _device(self):
        return next(self.decoder.parameters()).device

    def _batch_observations_and_actions(self, path_obs, path_actions, encoded_instructions):
        """speaker.py:68-121."""
        if 'feature' not in path_obs[0][0]:
            return self._batch_index_observations_and_actions(path_obs, path_actions, encoded_instructions)
        seq_lengths = np.array([len(a) for a in path_actions])
        Tp = int(seq_lengths.max())
        B = len(path_obs)
        dim = path_obs[0][0]['action_embedding'].shape[-1]
        fshape = path_obs[0][0]['feature'][0].shape
        mask = np.ones((B, Tp), np.uint8)
        acts = [np.zeros((B, dim), np.float32) for _ in range(Tp)]
        feats = [np.zeros((B,) + fshape, np.float32) for _ in range(Tp)]
        for i, (obs, actions) in enumerate(zip(path_obs, path_actions)):
            assert len(obs) == len(actions) + 1
            mask[i, :len(actions)] = 0
            for t, (ob, a) in enumerate(zip(obs[:-1], actions)):
                assert a >= 0
                feats[t][i] = ob['feature'][0]
                acts[t][i] = ob['action_embedding'][a]
        dev = self._device()
        to = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
        return ([obs[0] for obs in path_obs], [to(f) for f in feats], [to(a) for a in acts],
                to(mask), list(seq_lengths), encoded_instructions, list(range(B)))

    def _batch_index_observations_and_actions(self, path_obs, path_actions, encoded_instructions):
        """The same tensors from INDEX-FORM observations (what the beam search's encoder pass needs on an env that
        carries its feature store): per path step the panorama and the chosen action's embedding gathered from the
        store on the device (sf_gather_panorama, sf_gather_actions); padded steps are zero, as on the dense path."""
        store = self._env_store()
        if store is None:
            raise RuntimeError('index-form observations need a features.FeatureStore (env.image_features_list[0].store '
                               'or speaker.store)')
        seq_lengths = np.array([len(a) for a in path_actions])
        Tp, B = int(seq_lengths.max()), len(path_obs)
        mask = np.ones((B, Tp), np.uint8)
        vp, view, act_view = (np.zeros((Tp, B), np.int32) for _ in range(3))
        act = np.zeros((Tp, B), np.int32)         # 1: candidate 1 of the [stop, chosen action] list gather_actions reads
        heading, elevation = np.zeros((Tp, B), np.float64), np.zeros((Tp, B), np.float64)
        for i, (obs, actions) in enumerate(zip(path_obs, path_actions)):
            assert len(obs) == len(actions) + 1
            mask[i, :len(actions)] = 0
            for t, (ob, a) in enumerate(zip(obs[:-1], actions)):
                assert a >= 0
                vp[t, i], view[t, i] = ob['vp_row'], ob['viewIndex']
                if a > 0:
                    act[t, i] = 1
                    d = ob['adj_loc_list'][a]
                    act_view[t, i], heading[t, i], elevation[t, i] = d['absViewIndex'], d['rel_heading'], d['rel_elevation']
        from .features import cand_sincos
        dev = store.device
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        vp_d, view_d, av_d, act_d = to(vp), to(view), to(act_view), to(act)
        sc_d = to(cand_sincos(heading, elevation))
        pad = to(mask.T.astype(bool))
        feats, acts = [], []
        for t in range(Tp):
            f = store.gather_panorama(vp_d[t], view_d[t])
            feats.append(f.masked_fill_(pad[t][:, None, None], 0.0))
            acts.append(store.gather_actions(vp_d[t], av_d[t], sc_d[t], act_d[t]))     # (action 0 / padding: zeros)
        return ([obs[0] for obs in path_obs], feats, acts, to(mask), list(seq_lengths), encoded_instructions,
                list(range(B)))

    def _env_store(self):
        feats = getattr(self.env, 'image_features_list', None) or [None]
        return getattr(feats[0], 'store', None) or getattr(self, 'store', None)

    # `sample` feedback over a vocabulary of more than 1024 words (trainval_vocab.txt: 1 086): drawn by the per-step glue
    # kernel over up to sf_speaker_sample_max_vocab() words (speaker.check_sample_vocab).  Off by default: such a pass
    # raises NotImplementedError, as it always has.
    wide_sample = False

    def _speaker_engine(self, store):
        """The agent's speaker.SpeakerEngine over `store` (kept between calls), with the agent's switches."""
        from . import speaker as spk
        if getattr(self, '_engine', None) is None or self._engine.store is not store:
            self._engine = spk.SpeakerEngine(self.encoder, self.decoder, store)
        self._engine.wide_sample = self.wide_sample
        return self._engine

    SCORE_CHUNK = 128          # rows of one persistent word-loop launch (csrc/sf_persist.hip)
    # large teacher-forced scoring sweeps: the full chunks as replayed graphs on two streams (speaker.SpeakerSweep) instead
    # of launch-by-launch issue: -3.5 ms per minibatch of 64 instructions once every (stream, path-step count) graph is
    # captured, ~0.3 s of captures before that (tools/pragmatic_scoring_ab.py): pays after ~85 minibatches.  Off by default.
    score_graphs = False

    @gc_paused
    def _score_on_device(self, path_obs, path_actions, encoded_instructions, feedback, store):
        """The same scoring over INDEX-FORM observations (no 'feature' / 'action_embedding' rows: an env that
        carries its feature store): the fused speaker engine (speaker.SpeakerEngine -- per path step visual
        attention + LSTMCell with in-kernel gathers, the word loop as one persistent launch in inference).  Results in
        the layout of the host path below.

        A large inference batch (the pragmatic re-ranking hands over ALL ~2 500 candidate routes of a minibatch at
        once, rational_follower.py:67-69) is walked in chunks of SCORE_CHUNK rows, each one persistent launch: the
        host packs chunk k + 1 while the device decodes chunk k, one download and one fault check at the end.  Rows
        are independent; the loss (a mean over ALL rows per step, up to the first step at which every row has ended,
        speaker.py:188-197) is re-assembled from the chunks' (sum, count) tables."""
        from . import speaker as spk
        import time
        marks = getattr(self, 'score_marks', None)       # tools/pragmatic_profile.py: wall-clock marks of the phases
        mark = (lambda name: marks.append((name, time.perf_counter()))) if marks is not None else (lambda name: None)
        mark('start')
        B = len(path_obs)
        # (a search's RouteObservations knows its instruction without building its dictionaries)
        instr_ids = [obs.instr_id if hasattr(obs, 'instr_id') else obs[0]['instr_id'] for obs in path_obs]
        pend = self.__dict__.pop('_pending_scores', None)
        if pend is not None:
            if pend.matches(path_obs, feedback) and not torch.is_grad_enabled():   # issued by the search itself: collect
                self.prefetch_hits = getattr(self, 'prefetch_hits', 0) + 1
                return self._finish_scores(pend, instr_ids, mark)
            torch.cuda.synchronize()                      # (not the routes it was issued for: let it drain, drop it)
        n = np.array([len(a) for a in path_actions], np.int32)
        # one row (vp_row, viewIndex, absViewIndex, rel_heading, rel_elevation, is_stop) per (observation, action) pair,
        # formed once per DISTINCT pair: the candidate routes of a search share their observation dictionaries
        seen = {}

        def pair_rows(lo, hi):                                        # [sum of n[lo:hi], 6], candidate-major
            rows = []
            for obs, actions in zip(path_obs[lo:hi], path_actions[lo:hi]):
                assert len(obs) == len(actions) + 1
                for t, a in enumerate(actions):
                    ob = obs[t]
                    k = (id(ob), a)
                    r = seen.get(k)
                    if r is None:
                        assert a >= 0
                        if a > 0:
                            d = ob['adj_loc_list'][a]
                            r = (ob['vp_row'], ob['viewIndex'], d['absViewIndex'], d['rel_heading'], d['rel_elevation'], 0.0)
                        else:
                            r = (ob['vp_row'], ob['viewIndex'], 0, 0.0, 0.0, 1.0)
                        seen[k] = r
                    rows.append(r)
            return np.array(rows, np.float64).reshape(-1, 6)
        return self._score_index_routes(n, pair_rows, encoded_instructions, instr_ids, feedback, store, mark)

    def _score_index_routes(self, n, pair_rows, encoded_instructions, instr_ids, feedback, store, mark=lambda name: None):
        """The scoring pass over routes in INDEX FORM: n [routes] steps each, pair_rows(lo, hi) = the [sum n[lo:hi], 6] rows
        (vp_row, viewIndex, absViewIndex, rel_heading, rel_elevation, is_stop) of routes lo..hi-1, route-major."""
        from . import speaker as spk
        B = len(n)
        self._speaker_engine(store)
        eng = self._engine
        training = self.decoder.training
        chunked = B > 2 * self.SCORE_CHUNK and not training and not torch.is_grad_enabled() and eng.group is None
        if chunked:          # (pairs per chunk: formed while the device decodes the previous one)
            return self._finish_scores(self._issue_scores(n, pair_rows, encoded_instructions, feedback, store, mark),
                                       instr_ids, mark)
        S = self._score_steps(encoded_instructions, feedback)
        batch = spk.DeviceSpeakerBatch.from_synth(self._index_batch(n, pair_rows, encoded_instructions, 0, B),
                                                  device=store.device, max_length=self.instruction_len)
        st = eng.run(batch, S, feedback, train=training)                   # (fault check and re-issue inside)
        both = torch.cat((st.words[1:].to(torch.float32), st.step_scores), dim=0).cpu().numpy()   # (the one host sync)
        mark('downloaded')
        return self._score_outputs(instr_ids, both, S, st.loss, None, store.device, mark)

    def _score_steps(self, encoded_instructions, feedback):
        S = self.instruction_len
        if feedback == 'teacher':
            # the reference's loop ends once every row has ended (speaker.py:199-200): with teacher forcing that is the
            # longest instruction's EOS -- steps behind it add nothing to any score or to the loss
            S = max(1, min(S, max(len(e_) for e_ in encoded_instructions) + 1))
        return S

    @staticmethod
    def _index_batch(n, rows_of, encoded_instructions, lo, hi):
        """synth.SpeakerBatch (index form, speaker.py:68-121) of routes lo..hi-1: rows_of(lo, hi) = their [sum n, 6]
        (vp_row, viewIndex, absViewIndex, rel_heading, rel_elevation, is_stop) rows, route-major."""
        from . import synth
        m = n[lo:hi]
        Tp, Bc = int(m.max()), hi - lo
        t_of, owner = _ragged(m)
        at = t_of * Bc + owner
        part = rows_of(lo, hi)

        def grid(col, dt, fill=0):
            out = np.full(Tp * Bc, fill, dt)
            out[at] = part[:, col]
            return out.reshape(Tp, Bc)
        return synth.SpeakerBatch(instr=list(encoded_instructions[lo:hi]), path_len=m, vp=grid(0, np.int32),
                                  view=grid(1, np.int32), act_view=grid(2, np.int32), act_heading=grid(3, np.float64),
                                  act_elevation=grid(4, np.float64), act_is_stop=grid(5, np.float64, 1.0) != 0)

    def _issue_scores(self, n, rows_of, encoded_instructions, feedback, store, mark=lambda name: None):
        """Issues the chunked scoring sweep (no host sync) and returns what _finish_scores needs to collect it."""
        from . import speaker as spk
        self._speaker_engine(store)
        eng = self._engine
        B = len(n)
        S = self._score_steps(encoded_instructions, feedback)

        def staged_batch(k, lo, hi):
            """Chunk k through ONE pinned staging slice and ONE asynchronous H2D copy (a pageable `.to(device)` is a
            blocking copy: it would wait for the previous chunk's launches and serialise host and device)."""
            sb = self._index_batch(n, rows_of, encoded_instructions, lo, hi)
            Tp, Bc = sb.vp.shape
            nbytes = spk.packed_layout(Bc, Tp, self.instruction_len)['bytes']
            pin, dev_buf = self._staging(store.device, k, nbytes)
            spk.pack_speaker_batch(sb, pin.numpy(), Lmax=self.instruction_len, Tp=Tp)
            dev_buf[:nbytes].copy_(pin[:nbytes], non_blocking=True)
            return spk.batch_from_packed(dev_buf, Bc, Tp, Lmax=self.instruction_len, row0=lo)

        def sweep():
            parts = []
            for k, lo in enumerate(range(0, B, self.SCORE_CHUNK)):
                st = eng.score(staged_batch(k, lo, min(lo + self.SCORE_CHUNK, B)), S, feedback, train=False)
                parts.append((st.words[1:].to(torch.float32), st.step_scores, st.sum_cnt))
            return parts
        pend = _PendingScores()
        pend.B, pend.S, pend.feedback, pend.store, pend.sweep, pend.site = B, S, feedback, store, sweep, eng.site_next
        pend.graphs = None
        n_full = B // self.SCORE_CHUNK
        if self.score_graphs and feedback == 'teacher' and n_full >= 4 and eng.persistent and eng.group is None:
            # the full chunks as replayed graphs on two streams (speaker.SpeakerSweep: one captured pass per stream and
            # path-step count; the encoder steps of one chunk run beside the other stream's word recurrence), the
            # remainder issued launch by launch behind them
            key = (id(store), S, self.instruction_len, self.wide_sample)
            sw = self.__dict__.setdefault('_score_sweeps', {}).get(key)
            if sw is None or sw.enc is not self.encoder or sw.dec is not self.decoder:
                sw = self._score_sweeps[key] = spk.SpeakerSweep(self.encoder, self.decoder, store, self.SCORE_CHUNK, S,
                                                                feedback='teacher', Lmax=self.instruction_len, with_scores=True,
                                                                wide_sample=self.wide_sample)
            full = [self._index_batch(n, rows_of, encoded_instructions, lo, lo + self.SCORE_CHUNK)
                    for lo in range(0, n_full * self.SCORE_CHUNK, self.SCORE_CHUNK)]
            pend.graphs = (sw, sw.issue(full))
            lo = n_full * self.SCORE_CHUNK
            pend.parts = []
            if lo < B:
                st = eng.score(staged_batch(0, lo, B), S, feedback, train=False)
                pend.parts.append((st.words[1:].to(torch.float32), st.step_scores, st.sum_cnt))
        else:
            pend.parts = sweep()
        mark('issued')
        return pend

    def _finish_scores(self, pend, instr_ids, mark=lambda name: None):
        eng, dev = self._engine, pend.store.device
        swept = None
        if pend.graphs is not None:
            sw, handle = pend.graphs
            swept = sw.finish(handle, check_faults=False)                     # (waits for its two streams)
        bits = take_fault(dev)                                                # (one sync for the whole sweep)
        mark('device done')
        parts = pend.parts
        if bits:                                                              # a starved persistent launch: per-step kernels
            swept = None                                                      # (everything again, launch by launch)
            eng.site_next = pend.site
            parts = reissue_per_step(eng, eng, dev, 'a scoring sweep', pend.sweep, bits)
        if swept is not None:
            w16, sc, cnt = swept                                              # [n,S,128] int16 / f32, [n,S,2]
            S_ = pend.S
            words_h = w16.transpose(1, 0, 2).reshape(S_, -1).astype(np.float32)
            scores_h = sc.transpose(1, 0, 2).reshape(S_, -1)
            sum_cnt = cnt.astype(np.float32).sum(0)
            if parts:
                tail = torch.cat((parts[0][0], parts[0][1]), dim=0).cpu().numpy()
                words_h = np.concatenate((words_h, tail[:S_]), axis=1)
                scores_h = np.concatenate((scores_h, tail[S_:]), axis=1)
                # (float32 sums chunk by chunk, as the stacked device sum does)
                sum_cnt = sum_cnt + parts[0][2].cpu().numpy()
            both = np.concatenate((words_h, scores_h), axis=0)
        else:
            both = torch.cat((torch.cat([p_[0] for p_ in parts], dim=1), torch.cat([p_[1] for p_ in parts], dim=1)),
                             dim=0).cpu().numpy()
            sum_cnt = torch.stack([p_[2] for p_ in parts]).sum(0).cpu().numpy()        # [S,2]: all rows
        mark('downloaded')
        return self._score_outputs(instr_ids, both, pend.S, None, sum_cnt, dev, mark)

    def _score_outputs(self, instr_ids, both, S, loss, sum_cnt, device, mark=lambda name: None):
        B = len(instr_ids)
        words, sc = both[:S].T.astype(np.int64), np.ascontiguousarray(both[S:].T)                  # [B,S] each
        is_eos = words == EOS
        m_all = np.where(is_eos.any(1), is_eos.argmax(1) + 1, S)           # up to and including the first EOS
        if loss is None:
            # speaker.py:188-197 over the whole batch: step means up to and including the first step at which every row
            # has produced EOS, summed in step order in float32 (what sf_speaker_loss_finalize does for one batch)
            last = int(m_all.max()) - 1
            total = np.float32(0)
            for t in range(last + 1):
                if sum_cnt[t, 1] > 0:
                    total = np.float32(total + np.float32(sum_cnt[t, 0] / sum_cnt[t, 1]))
            loss = torch.tensor(float(total), device=device)
        totals = np.cumsum(sc, axis=1, dtype=np.float32)                   # (sequential float32 partial sums)
        tok = getattr(self.env, 'tokenizer', None)
        ends = m_all.tolist()
        last = totals[np.arange(B), m_all - 1].tolist()
        outputs = [_ScoredInstruction(instr_ids[i], last[i], words[i], sc[i], ends[i], tok) for i in range(B)]
        mark('outputs')
        return outputs, loss

    def route_scores_hook(self, feedback='teacher'):
        """For Seq2SeqAgent.candidates_hook (frontier.state_factored_search): the search hands over its completed routes
        in index form -- n [routes] steps each, rows [sum n, 6], the instruction of every route -- the moment its last
        iteration is done, BEFORE it builds their result dictionaries; the scoring sweep is issued right there, so the
        device decodes while the host builds ~2 500 dictionaries.  The hook returns `bind`: called with the routes'
        observation lists once they exist; the next _score_obs_actions_and_instructions over exactly those lists
        collects the scores instead of issuing them again (rational_follower.py:67-69 is that call)."""
        def hook(n, rows, instructions):
            store = self._env_store()
            if store is None or len(n) <= 2 * self.SCORE_CHUNK or self.decoder.training:
                return None
            stale = self.__dict__.pop('_pending_scores', None)
            if stale is not None:
                torch.cuda.synchronize()
            self._speaker_engine(store)
            if self._engine.group is not None:
                return None
            first = np.concatenate(([0], np.cumsum(n)))
            with torch.no_grad():       # (an inference sweep; a caller that wants gradients does not collect it)
                pend = self._issue_scores(np.asarray(n, np.int32), lambda lo, hi: rows[first[lo]:first[hi]], instructions,
                                          feedback, store)

            def bind(obs_lists):
                pend.obs_lists = list(obs_lists)
                self._pending_scores = pend
            return bind
        return hook

    def _staging(self, device, k, nbytes):
        """Pinned host / device staging buffers of chunk k of a chunked scoring pass (kept across calls; one pair per
        chunk, so that a chunk's buffer is never rewritten while its copy or its kernels are in flight)."""
        pool = self.__dict__.setdefault('_stage_pool', [])
        while len(pool) <= k:
            pool.append(None)
        if pool[k] is None or pool[k][0].numel() < nbytes or pool[k][1].device != device:
            cap = max(nbytes, 1 << 17)
            pool[k] = (torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.empty(cap, dtype=torch.uint8, device=device))
        return pool[k]

    def _score_obs_actions_and_instructions(self, path_obs, path_actions, encoded_instructions,
                                            feedback):
        """speaker.py:123-202."""
        assert len(path_obs) == len(path_actions) == len(encoded_instructions)
        if 'feature' not in path_obs[0][0]:
            store = self._env_store()
            if store is None:
                raise RuntimeError('index-form observations need a features.FeatureStore (env.image_features_list[0].store '
                                   'or speaker.store)')
            return self._score_on_device(path_obs, path_actions, encoded_instructions, feedback, store)
        if feedback == 'sample':                              # (before the encoder runs: nothing is launched for a refusal)
            from .speaker import check_sample_vocab
            check_sample_vocab(self.decoder.vocab_size, self.wide_sample)
        start_obs, feats, acts, path_mask, _, encoded_instructions, perm = \
            self._batch_observations_and_actions(path_obs, path_actions, encoded_instructions)
        dev = self._device()
        instr_seq, _, _ = batch_instructions_from_encoded(encoded_instructions, self.instruction_len,
                                                         device=dev)
        B = len(start_obs)
        ctx, h, c = self.encoder(acts, feats)
        w_t = torch.full((B,), BOS, dtype=torch.int64, device=dev)
        ended = np.array([False] * B)
        ended_dev = torch.zeros(B, dtype=torch.uint8, device=dev)
        outputs = [{'instr_id': start_obs[i]['instr_id'], 'word_indices': [], 'scores': []}
                   for i in range(B)]
        loss = 0
        seq_scores = torch.zeros(B, device=dev)
        for t in range(self.instruction_len):
            h, c, alpha, logit = self.decoder(w_t.view(-1, 1), h, c, ctx, path_mask)
            target = instr_seq[:, t].contiguous()
            self._sample_count += 1
            nll, live, w_t, score = _SpeakerGlueFn.apply(logit, target, FEEDBACK[feedback],
                                                         ended_dev, PAD, EOS, (self._sample_seed, self._sample_count))
            seq_scores = seq_scores + score
            loss = loss + nll.sum() / live.sum().clamp(min=1.0)
            words, sc, ss = w_t.tolist(), score.tolist(), seq_scores.tolist()
            for i in range(B):
                if not ended[i]:
                    outputs[i]['word_indices'].append(int(words[i]))
                    outputs[i]['score'] = float(ss[i])
                    outputs[i]['scores'].append(sc[i])
                if words[i] == EOS:
                    ended[i] = True
            if ended.all():
                break
        tok = getattr(self.env, 'tokenizer', None)
        for item in outputs:
            item['words'] = (tok.decode_sentence(item['word_indices'], break_on_eos=True, join=False)
                             if tok is not None else list(item['word_indices']))
        return outputs, loss

    index_gold_routes = True   # rollout(): the minibatch's gold routes from the navigation tables (nav.NavTable.gold_routes)
                               # instead of a lock-step walk of the host environment

    def rollout(self, load_next_minibatch=True):
        store = self._env_store()
        if (self.index_gold_routes and store is not None and getattr(self.env, 'host_table', 1) is None
                and hasattr(self.env, 'graphs')):
            # speaker.py:348-360 without the per-step host loop of env.py:823-848: teacher actions and transitions are
            # table look-ups over the whole minibatch, the routes arrive in index form (what the device consumes)
            from .nav import table_for
            self.env.reset(load_next_minibatch=load_next_minibatch)
            items = list(self.env.batch)
            n, rows = table_for(self.env, store).gold_routes(items, self.max_episode_len)
            first = np.concatenate(([0], np.cumsum(n)))
            outputs, loss = gc_paused(self._score_index_routes)(
                n, lambda lo, hi: rows[first[lo]:first[hi]], [it['instr_encoding'] for it in items],
                [it['instr_id'] for it in items], self.feedback, store)
            self.loss = loss
            self.losses.append(float(loss.detach()) if torch.is_tensor(loss) else float(loss))
            return outputs
        path_obs, path_actions, enc = self.env.gold_obs_actions_and_instructions(
            self.max_episode_len, load_next_minibatch=load_next_minibatch)
        outputs, loss = self._score_obs_actions_and_instructions(path_obs, path_actions, enc,
                                                                 self.feedback)
        self.loss = loss
        self.losses.append(float(loss.detach()) if torch.is_tensor(loss) else float(loss))
        return outputs

    # beam_search with its word loop on the device (search.DeviceSpeakerBeam: no host round trip per word, chunks of
    # `beam_chunk` word steps as replayed hipGraphs, or issued eagerly with beam_graphs = False).  Off by default.  Same
    # outputs as the host loop; inference only; beam_size <= 64 -- wider beams run the host loop and count a fallback.
    beam_on_device = False
    beam_chunk = 8
    beam_graphs = True
    beam_fallbacks = 0
    device_beam = None

    def beam_search(self, beam_size, path_obs, path_actions):
        """speaker.py:211-318 (search.py)."""
        from . import search
        if self.beam_on_device:
            if search.DeviceSpeakerBeam.supports(beam_size):
                return search.speaker_beam_search_device(self, beam_size, path_obs, path_actions)
            self.beam_fallbacks += 1
        return search.speaker_beam_search(self, beam_size, path_obs, path_actions)

    sweep_test_after = 30            # test(): minibatches (cumulative over calls) before the split is decoded as a sweep

    def _test_as_a_sweep(self):
        """test() over an index-form environment (speaker.py:397-414; data_augmentation_from_speaker.py's loop) through
        speaker.SpeakerSweep: the epoch's minibatches are drawn first (the same env.reset calls, the same use of
        `random` where the epoch wraps), their gold routes come from the navigation tables, and the device decodes them
        as replayed graphs on two streams -- packing, copies and decoding overlapped -- instead of one launch-by-launch
        pass per minibatch (4.6 -> 2.1 ms per minibatch of 100).  The graphs of a sweep (one per stream and route
        length) cost ~40 ms once: taken once this agent's test() calls have seen `sweep_test_after` minibatches (a
        data-augmentation pass at once, periodic validations from their second).  False: not applicable, the caller
        loops over rollout()."""
        store = self._env_store()
        if not (self.beam_size == 1 and self.index_gold_routes and store is not None and not self.decoder.training
                and self.feedback == 'argmax' and getattr(self.env, 'host_table', 1) is None
                and hasattr(self.env, 'graphs') and hasattr(self.env, 'data') and store.device.type == 'cuda'):
            return False
        B = self.env.batch_size
        n_batches = -(-len(self.env.data) // B)
        seen = self.__dict__.get('_test_minibatches', 0)
        self._test_minibatches = seen + n_batches
        if seen + n_batches < self.sweep_test_after:
            return False
        drawn = [items for _, items, _ in epoch_minibatches(self.env)]   # (speaker.py:404-413 over the items themselves)
        sweep = self._sweep_for(store, B)
        if self.device_routes:
            from .nav import table_for
            from .routes import RouteSet
            routes = RouteSet.from_items(table_for(self.env, store), [it for items in drawn for it in items])
            batches = routes.pack(B, self.instruction_len, chunk=self.device_routes_chunk, S=self.max_episode_len)
        else:
            batches = [self._routes_of(items, store)[0] for items in drawn]
        self._collect_sweep(sweep.run(batches), [[it['instr_id'] for it in items] for items in drawn], store)
        return True

    def _sweep_for(self, store, B):
        """The agent's speaker.SpeakerSweep for minibatches of B routes over `store`, kept between calls."""
        from . import speaker as spk
        key = (id(store), B, self.instruction_len, self.wide_sample)
        cached = self.__dict__.get('_test_sweep')
        if cached is None or cached[0] != key:
            cached = self._test_sweep = (key, spk.SpeakerSweep(self.encoder, self.decoder, store, B, self.instruction_len,
                                                               feedback='argmax', Lmax=self.instruction_len,
                                                               with_scores=True, wide_sample=self.wide_sample), store)
        return cached[1]

    def _collect_sweep(self, swept, ids_of, store):
        """The result dictionaries and losses of a finished sweep: minibatch k holds the instructions ids_of[k]."""
        words, scores, cnt = swept
        S = self.instruction_len
        for k, ids in enumerate(ids_of):
            both = np.concatenate((words[k].astype(np.float32), scores[k]), axis=0)
            outputs, loss = self._score_outputs(ids, both, S, None, cnt[k], store.device)
            self.loss = loss
            self.losses.append(float(loss))
            for result in outputs:
                if result['instr_id'] not in self.results:
                    self.results[result['instr_id']] = result

    # test()'s sweep over blocks packed ON THE DEVICE (routes.RouteSet.from_items(...).pack: two sf_nav_routes launches and
    # one host sync for the whole split, one D2D copy per minibatch) instead of gold_routes + pack_speaker_batch + one
    # H2D copy per minibatch.  Same staging bytes, same words.  Off by default.
    device_routes = False
    device_routes_chunk = None       # minibatches per device buffer (routes.PACK_CHUNK)

    def augment(self, routes, batch_size=100):
        """data_augmentation_from_speaker.py:35-82 without an environment: greedy instructions for every route of a
        routes.RouteSet (minibatches of `batch_size` in the set's order, a short last one filled from the front), decoded
        as ONE sweep over blocks packed on the device.  Returns what test() returns, keyed by instr_id;
        `routes.replaced_items(results)` is the split with the generated instructions."""
        store = self._env_store()
        if store is None or store.device.type != 'cuda':
            raise RuntimeError('Seq2SeqSpeaker.augment needs a feature store on the GPU (agent.store)')
        self.feedback, self.beam_size = 'argmax', 1
        for m in (self.encoder, self.decoder):
            m.eval()
        self.losses, self.results = [], {}
        packed = routes.pack(batch_size, self.instruction_len, chunk=self.device_routes_chunk, S=self.max_episode_len)
        ids = np.asarray(routes.instr_ids, object)[packed.route].reshape(len(packed), batch_size)
        self._collect_sweep(self._sweep_for(store, batch_size).run(packed), [row.tolist() for row in ids], store)
        return self.results

    def test(self, use_dropout=False, feedback='argmax', allow_cheat=False, beam_size=1):
        if not allow_cheat:
            assert feedback in ['argmax', 'sample']
        self.feedback = feedback
        for m in (self.encoder, self.decoder):
            m.train() if use_dropout else m.eval()
        self.beam_size = beam_size
        self.env.reset_epoch()
        self.losses = []
        self.results = {}
        if self._test_as_a_sweep():
            return self.results
        with torch.no_grad():
            return self._test_loop()

    def _test_loop(self):
        looped = False
        while True:
            for result in self.rollout():
                if result['instr_id'] in self.results:
                    looped = True
                else:
                    self.results[result['instr_id']] = result
            if looped:
                break
        return self.results

    train_without_outputs = True     # train(): forward and backward issued back to back, ONE host sync per iteration

    def _routes_of(self, items, store):
        """Host side of a training minibatch: its gold routes from the navigation tables, in the index form the device
        consumes (synth.SpeakerBatch), and the number of word steps."""
        from .nav import table_for
        n, rows = table_for(self.env, store).gold_routes(items, self.max_episode_len)
        first = np.concatenate(([0], np.cumsum(n)))
        enc = [it['instr_encoding'] for it in items]
        return (self._index_batch(n, lambda lo, hi: rows[first[lo]:first[hi]], enc, 0, len(items)),
                self._score_steps(enc, self.feedback))

    def _train_iteration_on_index_routes(self):
        """speaker.py:376-395's rollout + backward for train(), which reads nothing but the loss: the scoring pass and its
        backward are issued back to back (no download of words and scores, no result dictionaries, no sync between
        them), the NEXT minibatch's routes are formed while the device works (peeked, not drawn), and the fault word of
        the persistent launches is read once, where the loss is read; a fault re-issues the SAME minibatch on the
        per-step kernels.  Same kernels, same dropout sites as `rollout()` + `loss.backward()`.  False: not applicable
        (dense environment, row-sharded engine): the caller takes that path."""
        store = self._env_store()
        if not (self.train_without_outputs and self.index_gold_routes and store is not None
                and getattr(self.env, 'host_table', 1) is None and hasattr(self.env, 'graphs')):
            return False
        from . import speaker as spk
        self._speaker_engine(store)
        eng, dev = self._engine, store.device
        if eng.group is not None:
            return False
        self.env.reset()
        items = list(self.env.batch)
        ahead, prep = self.__dict__.pop('_routes_ahead', None), None
        if (ahead is not None and ahead[0] == self.feedback and len(ahead[1]) == len(items)
                and all(a is b for a, b in zip(ahead[1], items))):
            prep = ahead[2]
        sb, S = prep if prep is not None else self._routes_of(items, store)
        batch = spk.DeviceSpeakerBatch.from_synth(sb, device=dev, max_length=self.instruction_len)
        take_fault(dev)                                       # (whatever an earlier pass left behind is not ours)
        site = eng.site_next
        st = eng.score(batch, S, self.feedback, train=True)
        st.loss.backward()
        peek = getattr(self.env, 'peek_next_minibatch', None)
        nxt = peek(False) if peek is not None else None
        if nxt is not None:
            self._routes_ahead = (self.feedback, nxt, self._routes_of(nxt, store))
        bits = take_fault(dev)                                # the iteration's host sync
        if bits:
            for m in (self.encoder, self.decoder):
                for p_ in m.parameters():
                    if p_.grad is not None:
                        p_.grad.zero_()
            eng.site_next = site

            def again():
                st = eng.score(batch, S, self.feedback, train=True)
                st.loss.backward()
                return st
            st = reissue_per_step(eng, eng, dev, 'a training iteration', again, bits)
        self.loss = st.loss
        self.losses.append(float(st.loss.detach()))
        return True

    def train(self, encoder_optimizer, decoder_optimizer, n_iters, feedback='teacher'):
        assert feedback in self.feedback_options
        self.feedback = feedback
        self.encoder.train()
        self.decoder.train()
        self.losses = []
        for _ in range(1, n_iters + 1):
            encoder_optimizer.zero_grad()
            decoder_optimizer.zero_grad()
            if self._train_iteration_on_index_routes():
                encoder_optimizer.step()
                decoder_optimizer.step()
                continue
            self.rollout()
            self.loss.backward()
            # teacher-forced passes run their recurrence (forward and backward) as persistent launches since round 5: a
            # starved BACKWARD has poisoned the gradients -- never step on them; train this iteration on the next
            # minibatch with the per-step kernels instead (the forward's own check sits inside SpeakerEngine.run)
            dev = next(self.decoder.parameters()).device
            bits = fault_bits(dev)
            if bits:
                encoder_optimizer.zero_grad()
                decoder_optimizer.zero_grad()
                self.losses.pop()
                eng = getattr(self, '_engine', None)

                def again():
                    self.rollout()
                    self.loss.backward()
                reissue_per_step(eng, eng, dev, 'a training iteration', again, bits)
            encoder_optimizer.step()
            decoder_optimizer.step()

    def _encoder_and_decoder_paths(self, base_path):
        return base_path + '_enc', base_path + '_dec'

    def save(self, path):
        ep, dp = self._encoder_and_decoder_paths(path)
        torch.save(self.encoder.state_dict(), ep)
        torch.save(self.decoder.state_dict(), dp)

    def load(self, path, **kwargs):
        ep, dp = self._encoder_and_decoder_paths(path)
        self.encoder.load_state_dict(torch.load(ep, **kwargs))
        self.decoder.load_state_dict(torch.load(dp, **kwargs))
