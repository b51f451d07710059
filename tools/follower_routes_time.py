"""What follower pre-training on a routes.RouteSet costs per iteration through `Seq2SeqAgent.train_on_routes` (minibatches
packed on the device by sf_nav_follower_batches, one D2D copy each) against `Seq2SeqAgent.train` over an R2RIndexEnv of
the same items (host_arrays_for + one pinned H2D copy each, prepared under the running replay): routes enumerated over
the full 90-scan world the package ships (data/r2r_connectivity.npz), a sample of --routes of them with random
instructions of 10 .. 60 words, minibatches of 100, 80 words, teacher feedback, optim.FusedAdam.

One process and ONE agent (both loops replay the same captured graph): after 20 iterations of each, 200 timed iterations
per run, 5 runs of each taking turns; median, min and max of the runs.  Beside them
  host   milliseconds per minibatch of DeviceNavBatch.host_arrays_for(fixed=True) (50 minibatches)
  device microseconds per minibatch of RouteSet.pack_follower over 200 minibatches: the kernel's own time (the
         library's launch timer, _lib.kernel_profile: events around the launch) / 200, and, as an upper bound, events
         around the WHOLE call (epoch order, uploads of order and offsets, launch, the download of err / col_*) / 200
Feature rows wrap over a 2 048-row synthetic table (no time measured here depends on the values).  Information: nothing
is gated on it.

    python tools/follower_routes_time.py [--routes N] [--out profiles/follower_routes_sweep.txt]

--train-only [--tree DIR]: `train()` alone, with the same setup, from the package in DIR (default: this tree) -- the
baseline on another commit, whose checkout need not have this tool or anything of RouteSet's follower side:

    python tools/follower_routes_time.py --train-only --tree ../parent_checkout"""
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--tree' in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, ROOT)
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
from speaker_follower_amd import agents, env as E, evaluation, features, model, nav, nav_data, optim, routes, synth   # noqa: E402
from speaker_follower_amd.build import build_sim                             # noqa: E402

RUNS, ITERS, WARM, BATCH, WORDS, EPISODE, TABLE_ROWS = 5, 200, 20, 100, 80, 10, 2048


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


N_ROUTES, out_path, TRAIN_ONLY = arg('--routes', 30000), arg('--out', ''), '--train-only' in sys.argv
assert os.path.dirname(os.path.dirname(os.path.abspath(agents.__file__))) == ROOT, 'the package is not the one of --tree'
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


build_sim(verbose=False)
geo = nav_data.load_geometry()
scans = sorted(geo)
conn = nav_data.connectivity_dir(scans=scans)
row_of, n = {}, 0
for s in scans:
    for v, inc in zip(geo[s]['ids'], geo[s]['included']):
        if inc:
            row_of[s + '_' + v] = n % TABLE_ROWS
            n += 1
world = E.R2RIndexEnv([], row_of, conn, batch_size=BATCH, scans=scans)
dev = torch.device('cuda', 0)
table = nav.NavTable(world, types.SimpleNamespace(device=dev))
every = routes.RouteSet.enumerate(table, evaluation.DistanceTable(world.graphs))
split = every.sample(min(N_ROUTES, len(every)), 1)
rng = np.random.default_rng(2)
d = synth.FULL
enc_ids = [rng.integers(4, d.vocab, k) for k in rng.integers(10, 61, len(split))]
items = [dict(it, instr_encoding=e) for it, e in zip(split.items(), enc_ids)]
asked = ' --train-only' * TRAIN_ONLY + (' --tree %s' % sys.argv[sys.argv.index('--tree') + 1] if '--tree' in sys.argv else '')
say('python tools/follower_routes_time.py%s   (one MI355X; full world: %d scans, %d viewpoints, %d eligible pairs, %d routes; '
    'minibatches of %d, %d words, hop rows of %d; %d iterations after %d, median of %d runs, taking turns)'
    % (asked, len(scans), n, len(every), len(split), BATCH, WORDS, max(table.scan_rows.values()), ITERS, WARM, RUNS))

# ---- the two ways to a minibatch, alone
if not TRAIN_ONLY:
    split = split.with_instructions(enc_ids)
    t0 = time.perf_counter()
    for i in range(50):
        mb = sorted(items[i * BATCH:(i + 1) * BATCH], key=lambda it: len(it['instr_encoding']), reverse=True)
        nav.DeviceNavBatch.host_arrays_for(table, mb, WORDS, True, fixed=True)
    say('host   DeviceNavBatch.host_arrays_for(fixed=True): %.3f ms per minibatch (50 minibatches)' % ((time.perf_counter() - t0) * 20))
    split.pack_follower(BATCH, WORDS, order=split.epoch_order(BATCH, ITERS, 0))  # (uploads the route and token arrays)
    from speaker_follower_amd import _lib
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with _lib.kernel_profile() as prof:
            blocks = split.pack_follower(BATCH, WORDS, order=split.epoch_order(BATCH, ITERS, 0))
        b.record()
        b.synchronize()
        kernel = [r for k, r in prof.rows.items() if 'follower_batches' in k]
        assert len(kernel) == 1 and kernel[0]['calls'] == 1, prof.rows
        say('device RouteSet.pack_follower: kernel %.2f us per minibatch (%d minibatches in 1 launch of %.1f us, %d bytes each); '
            'whole call, upper bound: %.2f us per minibatch'
            % (kernel[0]['total_us'] / ITERS, ITERS, kernel[0]['total_us'], blocks.bytes, 1e3 * a.elapsed_time(b) / ITERS))
    del blocks

# ---- through the agents' API
env = E.R2RIndexEnv(items, row_of, conn, batch_size=BATCH, scans=scans)
w_enc, w_dec = synth.follower_weights_peaky(303)
enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=w_enc['embedding.weight'])
dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
enc.load_state_dict({k: torch.tensor(v) for k, v in w_enc.items()})
dec.load_state_dict({k: torch.tensor(v) for k, v in w_dec.items()})
agent = agents.Seq2SeqAgent(env, '', enc.cuda(), dec.cuda(), episode_len=EPISODE, max_instruction_length=WORDS)
agent.store = features.FeatureStore(synth.feature_table(3, TABLE_ROWS))
agent.use_device_env(table)
oe = optim.FusedAdam([p for p in enc.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)
od = optim.FusedAdam([p for p in dec.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4)


def run(on_routes, iters, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if on_routes:
        agent.train_on_routes(split, oe, od, iters, feedback='teacher', batch_size=BATCH, seed=seed)
    else:
        agent.train(oe, od, iters, feedback='teacher')
    torch.cuda.synchronize()
    assert len(agent.losses) == iters and np.isfinite(agent.losses).all()
    return 1e3 * (time.perf_counter() - t0) / iters


modes = (False,) if TRAIN_ONLY else (False, True)
for on in modes:
    run(on, WARM, 0)
graph = agent._train_graph_state[1]
rows = {False: [], True: []}
for rep in range(RUNS):
    for on in modes:
        rows[on].append(run(on, ITERS, rep + 1))
assert agent._train_graph_state[1] is graph, 'the two loops did not share one captured graph'
for on, name in ((False, 'train() over the environment'), (True, 'train_on_routes()'))[:len(modes)]:
    r = rows[on]
    say('%-30s %.3f ms per iteration  (min %.3f  max %.3f of %d runs)' % (name, statistics.median(r), min(r), max(r), RUNS))
if not TRAIN_ONLY:
    say('train_on_routes includes its pack_follower calls (one launch and one host sync per window of %d minibatches)'
        % routes.PACK_CHUNK)
if out_path:
    with open(out_path, 'a' if TRAIN_ONLY else 'w') as f:
        f.write('\n'.join(lines) + '\n')
