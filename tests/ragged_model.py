"""numpy model of a ragged offline batch (zen_amd/ragged/zen_hip_ragged.h), driven by the oracle's streaming engine: every
clip zero-padded to the batch's longest pass-1 length, pass 1 with oracle.HPR, the per-clip splice, pass 2 run to the longest
clip's hop count, the shifted and trimmed results.  Shared by tests/test_ragged_model.py (which checks it against
oracle.HPRIOffline per clip) and tests/test_gpu_ragged.py (fixtures)."""
import numpy as np

FS = 44100.0


def clip(n, seed):
    """n samples: a sine, noise and clicks"""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) / FS
    x = 0.3 * np.sin(2 * np.pi * (330 + 37 * seed) * t) + 0.2 * rng.uniform(-1, 1, n)
    for s in range(100 + 13 * seed, n, 1777):
        x[s:s + 20] += 0.8
    return x.astype(np.float32)


def clips_for(lengths, seed=0):
    return [clip(n, seed + i) for i, n in enumerate(lengths)]


def padded(n, hop, lag):
    """hpss_chunk_padder (hps.cu:109-126): float ceil of a float quotient, plus `lag` chunks; in samples"""
    return (int(np.ceil(np.float32(n) / np.float32(hop))) + lag) * hop


def ragged_model(o, hop_h, hop_p, clips, soft=False, sse=False, splice=True, beta=2.0):
    """(list_harm, list_perc) of the batch; splice=False: plain zero padding, pass 2 reads the shifted sum and zeros."""
    e1 = o.HPR(FS, hop_h, beta, o.OUTPUT_HARMONIC | o.OUTPUT_PERCUSSIVE | o.OUTPUT_RESIDUAL, o.TIME_ANTICAUSAL)
    e2 = o.HPR(FS, hop_p, beta, o.OUTPUT_PERCUSSIVE, o.TIME_ANTICAUSAL)
    for e in (e1, e2):
        if soft:
            e.use_soft_mask()
        if sse:
            e.use_sse_filter()
    sh1, sh2 = e1.lag * hop_h, e2.lag * hop_p
    lens = [c.size for c in clips]
    row1 = max(padded(n, hop_h, e1.lag) for n in lens)
    row2 = max(padded(n, hop_p, e2.lag) for n in lens)
    harm, perc = [], []
    for c in clips:
        n = c.size
        if n == 0:
            harm.append(np.zeros(0, np.float32))
            perc.append(np.zeros(0, np.float32))
            continue
        x = np.zeros(row1, np.float32)
        x[:n] = c
        e1.reset_buffers()
        o1 = e1.process_stream(x)
        q = o1["P"] + o1["R"]                      # float32: one IEEE add
        p1c = padded(n, hop_h, e1.lag)
        in2 = np.zeros(max(row2, row1), np.float32)
        if splice:
            in2[:p1c - sh1] = q[sh1:p1c]
            in2[p1c - sh1:p1c] = q[p1c - sh1:p1c]    # what the reference's in-place shift leaves behind
        else:
            in2[:row1 - sh1] = q[sh1:]               # every row treated as a clip of the longest length
            in2[row1 - sh1:row1] = q[row1 - sh1:]
        e2.reset_buffers()
        p2 = e2.process_stream(in2[:row2])["P"]
        harm.append(o1["H"][sh1:sh1 + n].copy())
        perc.append(p2[sh2:sh2 + n].copy())
    return harm, perc


def oracle_per_clip(o, hop_h, hop_p, clips, soft=False, sse=False, beta=2.0):
    """what oracle.HPRIOffline.process gives for each clip alone"""
    ref = o.HPRIOffline(FS, hop_h, hop_p, beta, beta)
    if soft:
        ref.use_soft_mask()
    if sse:
        ref.use_sse_filter()
    harm, perc = [], []
    for c in clips:
        if c.size == 0:
            harm.append(np.zeros(0, np.float32))
            perc.append(np.zeros(0, np.float32))
            continue
        h, p, _ = ref.process(c)
        harm.append(h)
        perc.append(p)
    return harm, perc
