"""What `Seq2SeqSpeaker.test()` over a split of ENUMERATED routes costs with `device_routes` off and on: the
data-augmentation pass (data_augmentation_from_speaker.py, configs[2]) over routes.RouteSet.enumerate of the full
90-scan world the package ships (data/r2r_connectivity.npz), a sample of --routes of them (default 178 300, the size of
the reference's downloaded split; all of them if there are fewer), minibatches of 100, 80 words.

One process, after a warm-up turn of each, taking turns, median of 7 with min / max.  Per turn, beside the wall time:
  off  `host_pack_s` (SpeakerSweep: pack_speaker_batch into the pinned slots) and the seconds in NavTable.gold_routes
  on   the seconds in RouteSet.from_items and in RouteSet.pack (two launches per chunk, one host sync)
and once: the seconds to build NavTable.all_hops and to enumerate.  Feature rows wrap over a 2 048-row synthetic table
(3 GB otherwise; no time measured here depends on the values).  Information: nothing is gated on it.

    python tools/device_routes_time.py [--routes N] [--out profiles/device_routes_sweep.txt]"""
import os
import random
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                                 # noqa: E402
from speaker_follower_amd import agents, env as E, evaluation, features, model, nav, nav_data, routes, synth   # noqa: E402
from speaker_follower_amd.build import build_sim                             # noqa: E402

REPS, BATCH, WORDS, EPISODE, TABLE_ROWS = 7, 100, 80, 10, 2048


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


N_ROUTES, out_path = arg('--routes', 178300), arg('--out', '')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


class Clock:
    """Seconds spent inside a function, summed over its calls."""

    def __init__(self, owner, name):
        self.s, fn = 0.0, getattr(owner, name)

        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.s += time.perf_counter() - t0
        setattr(owner, name, timed)

    def take(self):
        s, self.s = self.s, 0.0
        return s


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
t0 = time.perf_counter()
table.all_hops()
t_hops = time.perf_counter() - t0
dist = evaluation.DistanceTable(world.graphs)
t0 = time.perf_counter()
every = routes.RouteSet.enumerate(table, dist)
t_enum = time.perf_counter() - t0
split = every.sample(min(N_ROUTES, len(every)), 1)
t0 = time.perf_counter()
items = split.items()
t_items = time.perf_counter() - t0
say('python tools/device_routes_time.py   (one MI355X; %d scans, %d viewpoints, %d eligible pairs (%d unreached), %d routes, '
    'minibatches of %d, %d words, median of %d, taking turns)' % (len(scans), n, len(every), every.unreached, len(items),
                                                                  BATCH, WORDS, REPS))
say('once: all_hops %.2f s (%d elements), enumerate %.3f s, items() %.2f s' % (t_hops, len(table.all_hops()), t_enum, t_items))

env = E.R2RIndexEnv(items, row_of, conn, batch_size=BATCH, scans=scans)
d = synth.FULL
w_enc, w_dec = synth.speaker_weights_peaky(404)
enc = model.SpeakerEncoderLSTM(d.feat, d.feat, d.hidden, 0.5)
dec = model.SpeakerDecoderLSTM(d.vocab, d.word, d.hidden, 0.5, glove=w_dec['embedding.weight'])
enc.load_state_dict({k: torch.tensor(v) for k, v in w_enc.items()})
dec.load_state_dict({k: torch.tensor(v) for k, v in w_dec.items()})
spk = agents.Seq2SeqSpeaker(env, '', enc.cuda().eval(), dec.cuda().eval(), WORDS, max_episode_len=EPISODE)
spk.store = features.FeatureStore(synth.feature_table(3, TABLE_ROWS))
spk.sweep_test_after = 0
env._nav_table = (spk.store, table, tuple(sorted(env.graphs)))               # (the table built above serves the env: same scans)
data0 = list(env.data)
clocks = dict(gold=Clock(nav.NavTable, 'gold_routes'), from_items=Clock(routes.RouteSet, 'from_items'),
              pack=Clock(routes.RouteSet, 'pack'))


def turn(on, with_words):
    env.data[:] = data0
    random.seed(17)
    spk.device_routes = on
    for c in clocks.values():
        c.take()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = spk.test(use_dropout=False, feedback='argmax')
    wall = time.perf_counter() - t0
    words = {k: tuple(v['word_indices']) for k, v in res.items()} if with_words else None
    return wall, spk._test_sweep[1].host_pack_s, {k: c.take() for k, c in clocks.items()}, words, len(spk.losses)


rows, first_words = {False: [], True: []}, {}
for rep in range(REPS + 1):                                                  # (the first round warms up: graphs, tables)
    for on in (False, True):
        wall, pack_s, parts, words, n_mb = turn(on, rep == 0)
        if rep == 0:
            first_words[on] = words
        else:
            rows[on].append((wall, pack_s, parts))
assert first_words[False] == first_words[True], 'device_routes changed the generated words'
med = lambda xs: statistics.median(xs)                                       # noqa: E731
for on in (False, True):
    wall = [r[0] for r in rows[on]]
    say('device_routes %-5s test() median %7.3f s  min %7.3f  max %7.3f   (%d minibatches: %.3f ms each)'
        % (on, med(wall), min(wall), max(wall), n_mb, 1e3 * med(wall) / n_mb))
    if on:
        say('    of which RouteSet.from_items %.3f s, RouteSet.pack %.3f s (lengths launch, one sync, pack launches), host_pack_s %.3f'
            % (med([r[2]['from_items'] for r in rows[on]]), med([r[2]['pack'] for r in rows[on]]), med([r[1] for r in rows[on]])))
    else:
        say('    of which NavTable.gold_routes %.3f s, host_pack_s %.3f s'
            % (med([r[2]['gold'] for r in rows[on]]), med([r[1] for r in rows[on]])))
say('fallbacks %d; the generated words are the same with the switch off and on' % spk._test_sweep[1].fallbacks)
if out_path:
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
