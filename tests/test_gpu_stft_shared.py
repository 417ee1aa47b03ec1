"""GPU tier: the kernels zen_amd/repet, repsim and nmf share through zen_amd/addon (stft_kernels.h, median_select.h).  Each
library compiles them into a code object of its own, so the three hold device kernels of one mangled name; with all three in
one process each must still launch its own.  A fresh child process per load order loads all three before any of them launches
anything, then runs one small separation each; every output is compared bit for bit with tests/repet_model.py,
repsim_model.py and nmf_model.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import nmf_model  # noqa: E402
import repet_model  # noqa: E402
import repsim_model  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("repet", "repsim", "nmf")
FS, NFFT, SAMPLES = 8000.0, 64, 300         # 300 samples are no multiple of the hop of 32: 11 frames, the last two partly padding
PERIOD, NUMBER, COMPONENTS, ITERATIONS = 2, 3, 2, 2
THRESHOLD, DISTANCE_S, HIGHPASS = 0.0, 1.0 / FS, 300.0     # neighbours one frame apart and more; the three lowest bins kept whole

CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
order = sys.argv[2].split(",")
fs, nfft, period, number, components, iterations, threshold, distance, highpass = (float(v) for v in sys.argv[4:13])
x = np.load(sys.argv[3])
mods = {n: importlib.import_module("zen_amd." + n) for n in order}
for n in order:
    mods[n].load()                      # all three are in the process before a kernel of any of them is launched
import zen_amd
zen_amd.init(0)
repet, repsim, nmf = mods["repet"], mods["repsim"], mods["nmf"]
out = {}
bg, fg, used = repet.Repet(fs, int(nfft), 1, x.size, highpass_hz=highpass).run(x, periods=[int(period)])
out["repet"] = {"background": bg, "foreground": fg, "used": np.asarray(used, np.float32)}
bg, fg, counts, idx = repsim.Repsim(fs, int(nfft), 1, x.size, threshold, distance, int(number), highpass).run(x, selection=True)
out["repsim"] = {"background": bg, "foreground": fg, "counts": counts.astype(np.float32), "idx": idx.astype(np.float32)}
W, H, stems = nmf.decompose(x, fs, int(components), int(nfft), int(iterations))
out["nmf"] = {"W": W, "H": H, "stems": stems}
print(json.dumps({n: {k: np.ascontiguousarray(v, np.float32).view(np.uint32).ravel().tolist() for k, v in o.items()} for n, o in out.items()}))
"""


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    rng = np.random.default_rng(64)
    t = np.arange(SAMPLES)
    x = (0.4 * np.sin(2 * np.pi * 0.11 * t) * (t % 64 < 40) + 0.2 * rng.uniform(-1, 1, SAMPLES)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("stft_shared") / "clip.npy")
    np.save(path, x)
    return x, path


@pytest.fixture(scope="module")
def want(clip, oracle):
    """the three models' outputs, computed once for both load orders"""
    oracle.lib()
    x = clip[0]
    m, F = repet_model.n_frames(x.size, NFFT // 2), NFFT // 2 + 1
    assert m == 11 and x.size % (NFFT // 2) != 0
    rp = repet_model.separate(x, FS, NFFT, PERIOD, highpass=HIGHPASS)
    rs = repsim_model.separate(x, FS, NFFT, THRESHOLD, DISTANCE_S, NUMBER, HIGHPASS)
    W0, H0 = nmf_model.initial(0, COMPONENTS, F, m)
    nm = nmf_model.process(x, NFFT, W0, H0, 0, ITERATIONS, list(range(COMPONENTS)), COMPONENTS)
    assert np.all(rs.counts == NUMBER), "every frame finds its three neighbours: the register median at its count of 3"
    return {"repet": {"background": bits(rp.background), "foreground": bits(rp.foreground), "used": bits(np.float32([PERIOD]))},
            "repsim": {"background": bits(rs.background), "foreground": bits(rs.foreground), "counts": bits(rs.counts.astype(np.float32)),
                       "idx": bits(rs.idx.astype(np.float32))},
            "nmf": {"W": bits(nm.W), "H": bits(nm.H), "stems": bits(nm.stems)}}


@pytest.mark.parametrize("order", (NAMES, NAMES[::-1]), ids=("repet_first", "nmf_first"))
def test_each_library_launches_its_own_copy_of_the_shared_kernels(clip, want, order):
    args = [FS, NFFT, PERIOD, NUMBER, COMPONENTS, ITERATIONS, THRESHOLD, DISTANCE_S, HIGHPASS]
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, ",".join(order), clip[1]] + [repr(float(v)) for v in args], stdout=subprocess.PIPE,
                       universal_newlines=True, check=True)
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for n in NAMES:
        assert sorted(got[n]) == sorted(want[n]), n
        for k in want[n]:
            assert got[n][k] == want[n][k], "%s: %s differs from tests/%s_model.py" % (n, k, n)
