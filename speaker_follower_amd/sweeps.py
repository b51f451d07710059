"""What the device sweeps over a test() epoch share (Evaluation.score_agent, SpeakerEvaluation.score_speaker,
Seq2SeqSpeaker._test_as_a_sweep): the walk over the environment and the way back after a faulting sweep.  The fault
words themselves are cleared and downloaded by runtime.clear_faults / runtime.download_faults.

Nothing here imports torch or the library."""
import random


def epoch_minibatches(env, sort=False):
    """The minibatches of one test() epoch, after the caller's `env.reset_epoch()`, as BaseAgent.test walks them
    (follower.py:145-188): `env.reset()` -- `env.reset(sort=True)` with `sort` -- until an id repeats.  Yields
    (k, items, fresh): minibatch k's items and, per item, whether its 'instr_id' is met for the first time (the first
    occurrence of an id wins).  The minibatch that holds a repeated id is the last one and is yielded whole: fresh ids
    behind the repeated one still count.  The environment is advanced when the NEXT minibatch is asked for, so a caller
    may launch per minibatch inside its loop; nothing but `env.reset` touches `random`."""
    seen, k, looped = set(), 0, False
    while not looped:
        if sort:
            env.reset(sort=True)
        else:
            env.reset()
        items = list(env.batch)
        fresh = []
        for it in items:
            fresh.append(it['instr_id'] not in seen)
            seen.add(it['instr_id'])
        looped = not all(fresh)
        yield k, items, fresh
        k += 1


def snapshot(env):
    """The environment's item order and the state of `random` before a walk: what `restore` puts back."""
    return list(env.data), random.getstate()


def restore(env, snap):
    """Undo a walk: a test() that follows walks what the sweep walked."""
    env.data[:] = snap[0]
    random.setstate(snap[1])
