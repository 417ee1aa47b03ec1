"""numpy model of a live session (zen_amd/live/zen_hip_live.h), driven by the oracle's streaming engine: two anticausal
oracle.HPR engines fed hop-block by hop-block as the samples arrive, state carried from push to push, the tail assembled at
finish.  What it keeps between calls does not grow with the stream: the partial block, the samples of H1 / P2 / the input
that are computed but not yet due, and four counters.  Shared by tests/test_live_model.py (which checks it against
oracle.HPRIOffline on the whole clip) and tests/test_gpu_live.py (delivery counts)."""
import numpy as np

from ragged_model import FS, clip, padded  # noqa: F401  (clip: re-exported for the tests)

GEOMETRIES = ((256, 64), (512, 128), (128, 128), (1024, 256))
F32 = np.float32


def lengths_for(hop_h):
    return [1, 63, hop_h, hop_h + 1, 3 * hop_h - 1, 7 * hop_h, 12 * hop_h + 5, 33 * hop_h + 17]


def random_pushes(n, hop_h, seed):
    """push sizes uniform in [0, 3 * hop_h) from a fixed seed, cut to sum to n; a push of nothing behind the first one"""
    rng = np.random.default_rng(seed)
    sizes, left = [], n
    while left:
        m = min(int(rng.integers(0, 3 * hop_h)), left)
        sizes.append(m)
        left -= m
    return sizes[:1] + [0] + sizes[1:]


def fixed_pushes(n, m):
    return [m] * (n // m) + ([n % m] if n % m else [])


def cases():
    """the 36 cases: (hop_h, hop_p, n, pushes, soft, sse)"""
    out = []
    for g, (hop_h, hop_p) in enumerate(GEOMETRIES):
        for i, n in enumerate(lengths_for(hop_h)):
            out.append((hop_h, hop_p, n, random_pushes(n, hop_h, 100 * g + i), False, False))
    out.append((256, 64, 5123, random_pushes(5123, 256, 900), True, False))
    out.append((256, 64, 5123, random_pushes(5123, 256, 901), False, True))
    out.append((256, 64, 5123, fixed_pushes(5123, 256), False, False))
    out.append((256, 64, 5123, fixed_pushes(5123, 100), False, False))
    return out


def case_id(c):
    hop_h, hop_p, n, pushes, soft, sse = c
    kind = "soft" if soft else "sse" if sse else "hard"
    return "%dx%d-n%d-%s-%dpushes" % (hop_h, hop_p, n, kind, len(pushes))


def delivered_after(pushed, hop_h, latency):
    """samples of each output a session has handed out once `pushed` samples are in: host arithmetic only"""
    return max(0, pushed // hop_h * hop_h - latency)


class Tail:
    """the samples of one stream from position `pos` on: appended at the end, dropped at the front"""

    def __init__(self):
        self.pos, self.buf = 0, np.zeros(0, F32)

    def append(self, x):
        self.buf = np.concatenate([self.buf, x.astype(F32)])

    def get(self, a, b):
        if a == b:
            return np.zeros(0, F32)
        assert self.pos <= a <= b <= self.pos + self.buf.size, (self.pos, a, b, self.buf.size)
        return self.buf[a - self.pos:b - self.pos].copy()

    def drop_to(self, a):
        if a > self.pos:
            self.buf = self.buf[a - self.pos:]
            self.pos = a


class LiveModel:
    def __init__(self, o, hop_h, hop_p, soft=False, sse=False, beta=2.0, keep_tail=True):
        self.e1 = o.HPR(FS, hop_h, beta, o.OUTPUT_HARMONIC | o.OUTPUT_PERCUSSIVE | o.OUTPUT_RESIDUAL, o.TIME_ANTICAUSAL)
        self.e2 = o.HPR(FS, hop_p, beta, o.OUTPUT_PERCUSSIVE, o.TIME_ANTICAUSAL)
        for e in (self.e1, self.e2):
            if soft:
                e.use_soft_mask()
            if sse:
                e.use_sse_filter()
        self.hop_h, self.hop_p, self.keep_tail = hop_h, hop_p, keep_tail
        self.lag_h, self.lag_p = self.e1.lag, self.e2.lag
        self.sh1, self.sh2 = self.lag_h * hop_h, self.lag_p * hop_p
        self.latency = self.sh1 + self.sh2
        self.reset()

    def reset(self):
        self.e1.reset_buffers()
        self.e2.reset_buffers()
        self.pushed = self.delivered = self.done1 = 0          # done1: samples pass 1 has consumed
        self.carry = np.zeros(0, F32)
        self.h1, self.p2, self.dry = Tail(), Tail(), Tail()     # H1 / P2 / input by stream position

    def produces(self, m):
        return delivered_after(self.pushed + m, self.hop_h, self.latency) - self.delivered

    def pending(self):
        return self.pushed - self.delivered

    def push(self, x):
        x = np.asarray(x, F32).reshape(-1)
        want = self.produces(x.size)
        self.dry.append(x)
        self.pushed += x.size
        xs = np.concatenate([self.carry, x])
        b = xs.size // self.hop_h
        self.carry = xs[b * self.hop_h:]
        if b:
            o1 = self.e1.process_stream(xs[:b * self.hop_h])
            q = o1["P"] + o1["R"]                               # float32: one IEEE add
            self.h1.append(o1["H"])
            in2 = q[max(self.sh1 - self.done1, 0):]             # in2[j] = Q[j + sh1]: the first sh1 samples of Q's life dropped
            self.done1 += b * self.hop_h
            if in2.size:
                self.p2.append(self.e2.process_stream(in2)["P"])
        d0, d1 = self.delivered, delivered_after(self.pushed, self.hop_h, self.latency)
        assert d1 - d0 == want
        out = (self.h1.get(d0 + self.sh1, d1 + self.sh1), self.p2.get(d0 + self.sh2, d1 + self.sh2), self.dry.get(d0, d1))
        if d1:
            self.h1.drop_to(d1 + self.sh1)
            self.p2.drop_to(d1 + self.sh2)
            self.dry.drop_to(d1)
        self.delivered = d1
        return out

    def finish(self):
        n, sh1, sh2 = self.pushed, self.sh1, self.sh2
        if n == 0:
            return tuple(np.zeros(0, F32) for _ in range(3))
        pad1, pad2 = padded(n, self.hop_h, self.lag_h), padded(n, self.hop_p, self.lag_p)
        s0 = self.done1
        assert s0 + sh1 <= pad1, "blocks already processed exceed what the padder asks for"
        xs = np.zeros(pad1 - s0, F32)
        xs[:self.carry.size] = self.carry
        o1 = self.e1.process_stream(xs)
        q = o1["P"] + o1["R"]                                   # Q[s0, pad1)
        self.h1.append(o1["H"])
        # pass 2's input from where it stands up to pad2: the shifted Q, then the last sh1 samples of Q again, then zeros
        t = np.arange(max(s0 - sh1, 0), pad2)
        in2 = np.zeros(t.size, F32)
        a = t < pad1 - sh1
        in2[a] = q[t[a] + sh1 - s0]
        if self.keep_tail:
            st = (t >= pad1 - sh1) & (t < pad1)
            in2[st] = q[t[st] - s0]
        self.p2.append(self.e2.process_stream(in2)["P"])
        j = np.arange(self.delivered, n)

        def mapped(tail, sh, pad):
            out = np.zeros(j.size, F32)
            a = j < pad - sh
            st = (j >= pad - sh) & (j < pad)
            assert np.all(j[a] + sh >= tail.pos) and np.all(j[st] >= tail.pos), "the end mapping names a sample that is gone"
            out[a] = tail.buf[j[a] + sh - tail.pos]
            out[st] = tail.buf[j[st] - tail.pos]
            return out
        out = (mapped(self.h1, sh1, pad1), mapped(self.p2, sh2, pad2), self.dry.get(self.delivered, n))
        self.reset()
        return out


def run(model, x, pushes):
    """the whole clip through push / finish: (harm, perc, dry, counts) with counts = what every call handed out"""
    parts, at = [], 0
    for m in pushes:
        parts.append(model.push(x[at:at + m]))
        at += m
    assert at == x.size
    parts.append(model.finish())
    outs = [np.concatenate([p[k] for p in parts]) for k in range(3)]
    return outs[0], outs[1], outs[2], [p[0].size for p in parts]
