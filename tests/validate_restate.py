"""numpy restatements of the validation kernels (lt_eval_head, lt_early_stop_update): the evaluation head in a chosen
precision and the early-stopping state rule word for word.  Shared by test_validate_cpu.py and test_validate_gpu.py."""
import numpy as np

STATE_WORDS = 8
BEST_LOSS, BEST_EPOCH, COUNTER, STOP_EPOCH, IMPROVED, SEEN = range(6)


def head(z, y, dtype=np.float64):
    """(mean loss as a Python float, confusion [C, C] int64) of logits ``z`` [n, C] against labels ``y``: per row
    ``(max + log(sum exp(z - max))) - z[y]`` with the classes added in order, predicted class = FIRST argmax, every step in
    ``dtype``; the mean is the sum of the row losses in ``dtype`` divided by n."""
    z = np.asarray(z, dtype=dtype)
    y = np.asarray(y).astype(np.int64)
    n, c = z.shape
    mx = z.max(axis=1)
    arg = z.argmax(axis=1)                     # numpy returns the first maximum
    s = np.zeros(n, dtype=dtype)
    for k in range(c):
        s = (s + np.exp(z[:, k] - mx)).astype(dtype)
    row = ((mx + np.log(s)).astype(dtype) - z[np.arange(n), y]).astype(dtype)
    loss = row.sum(dtype=dtype) / dtype(n)
    conf = np.bincount(y * c + arg, minlength=c * c).reshape(c, c).astype(np.int64)
    return float(loss), conf


def state_reset():
    s = np.zeros(STATE_WORDS, dtype=np.int32)
    s[BEST_EPOCH] = s[STOP_EPOCH] = -1
    return s


def state_update(s, loss, patience, epoch):
    """One epoch applied to the 8 state words (a copy is returned): EarlyStopping.__call__ with delta = 0 on fp32 losses."""
    s = s.copy()
    if s[STOP_EPOCH] >= 0:
        s[IMPROVED] = 0
        return s
    loss = np.float32(loss)
    best = s[BEST_LOSS:BEST_LOSS + 1].view(np.float32)[0]
    if s[SEEN] > 0 and loss > best:            # false for a tie and for a NaN on either side
        s[COUNTER] += 1
        s[IMPROVED] = 0
        if patience > 0 and s[COUNTER] >= patience:
            s[STOP_EPOCH] = epoch
    else:
        s[BEST_LOSS] = np.array([loss], dtype=np.float32).view(np.int32)[0]
        s[BEST_EPOCH] = epoch
        s[COUNTER] = 0
        s[IMPROVED] = 1
    s[SEEN] = 1
    return s


def run_state(losses, patience):
    """The states after each epoch of ``losses`` (epoch = index)."""
    s, out = state_reset(), []
    for e, l in enumerate(losses):
        s = state_update(s, l, patience, e)
        out.append(s)
    return out


def decide(losses, patience):
    """(best_epoch, stop_epoch) after the whole sequence."""
    s = run_state(losses, patience)[-1]
    return int(s[BEST_EPOCH]), int(s[STOP_EPOCH])


NAN = float("nan")
# (name, losses, patience, (best_epoch, stop_epoch) after the last epoch, counter after the last epoch)
HAND_SEQUENCES = [
    ("tie_resets", [1.0, 1.5, 1.0, 1.5, 1.5, 1.0, 2.0], 3, (5, -1), 1),         # equal losses improve and reset the counter
    ("nan_becomes_best", [1.0, 2.0, NAN, NAN, NAN, NAN], 2, (5, -1), 0),         # NaN > best and best > NaN are both false
    ("nan_first", [NAN, NAN, NAN], 1, (2, -1), 0),
    ("nan_then_finite", [1.0, NAN, 0.5, 0.75, 0.8], 2, (2, 4), 2),               # 0.5 > NaN is false too: as in the reference
                                                                                 # a NaN best holds only until the next loss
    ("patience_1", [1.0, 0.5, 0.75, 0.25], 1, (1, 2), 1),                        # stops at the first rise; frozen after it
    ("patience_longer", [1.0, 2.0, 3.0, 4.0], 10, (0, -1), 3),
    ("frozen_after_stop", [1.0, 2.0, 3.0, 0.1, 0.0, NAN, 5.0], 2, (0, 2), 2),    # nothing changes after the stop
    ("never_stop", [1.0, 2.0, 3.0, 4.0, 0.5, 0.6], 0, (4, -1), 1),               # patience 0: keep the best, never stop
]
