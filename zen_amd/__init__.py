"""zen_amd -- MI355X (gfx950) native HPSS engine behind sevagh/Zen's GPU-backend interface.

The product is the C-ABI shared library zen_amd/libzen_hip.so (sources in zen_amd/csrc, interface in
include/zen_hip.h) plus the C++ host mirror of the reference's libzen in zen_amd/libzen.  This package
is a thin ctypes binding used by tests/ and bench.py; it never falls back to a CPU path: if the HIP
library is missing or no GPU is present the calls raise.
"""
from .lib import (  # noqa: F401
    FREQUENCY, OUTPUT_HARMONIC, OUTPUT_PERCUSSIVE, OUTPUT_RESIDUAL, TIME_ANTICAUSAL, TIME_CAUSAL,
    BoxFilterGPU, DeviceBuffer, Event, FFTC2CWrapperGPU, HPR, HPRIOffline, HPRRealtime, IOGPU, MedianFilterGPU, PinnedHost,
    ZenHipError, ZgException, blockrun_set, blockrun_stats, debug_poke, device_name, init, load, memcheck, run_plan, set_option, synchronize,
)
# the add-on builders under the names their four modules had: `from zen_amd import pcm_build` keeps working
from .addon_build import beat as beat_build, cqt as cqt_build, live as live_build, multi as multi_build, nmf as nmf_build, pcm as pcm_build, pitch as pitch_build, ragged as ragged_build, repet as repet_build, repsim as repsim_build, resample as resample_build, tsm as tsm_build  # noqa: F401,E402
