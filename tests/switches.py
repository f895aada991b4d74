"""Every MI355_* environment switch that gr-clenabled_amd/csrc reads, classified.  A plain module (no fixtures): the table below, and the
scanners tests/test_switch_inventory.py compares it with.

A row: name -> (block, when, class, note).

when    "process"  read once per process (a `static` initialiser): only a fresh process sees a new value -- tests/test_switches_once_gpu.py
        "create"   read when a handle is created (or its taps are set)
        "call"     read at every launch
class   "alternative"  selects code the default routing never reaches
        "reroute"      moves a shape between kernels that are each reached elsewhere
        "identical"    INTEGRATION.md promises identical results: compared bit for bit with the default
        "tuning"       grid, tile or schedule size only
        "not_run"      never set by the suite's switch cases; the note says why

Every row that is not "not_run" is referenced by at least one case of tests/switch_cases.py (test_switch_inventory.py checks it).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gr-clenabled_amd", "csrc")
WHEN = ("process", "create", "call")
CLASSES = ("alternative", "reroute", "identical", "tuning", "not_run")

SWITCHES = {
    # ------------------------------------------------------------------------------------------------------------ host paths
    "MI355_NO_DIRECT": ("host", "process", "alternative", "staged copies for scheduler-sized calls"),
    "MI355_CHUNK_MB": ("host", "process", "tuning", "staging chunk of large host calls: many pieces"),
    "MI355_COPY_STREAM": ("host", "process", "alternative", "cached memcpy instead of streaming stores"),
    "MI355_COPY_THREADS": ("host", "process", "alternative", "staging copies on the calling thread alone"),
    "MI355_SPIN_US": ("host", "process", "tuning", "polling window of the direct path's wait; 0 = always sleep"),
    "MI355_SPIN": ("host", "create", "not_run", "sets the process-wide hipDeviceScheduleSpin flag: would change how every later test of the process waits"),
    "MI355_WG_PER_CU": ("host", "call", "tuning", "grid of every mi355_balanced_grid kernel"),
    "MI355_MATH_WG_PER_CU": ("mathop", "call", "tuning", "grid of the clMathOp family"),
    # ------------------------------------------------------------------------------------------------------------------ clFFT
    "MI355_CHIRPZ_FUSED": ("fft", "process", "alternative", "five-launch chirp-z path for m <= 16384"),
    "MI355_FFT_WHOLE_FRAME": ("fft", "process", "alternative", "8192 / 16384 points with the whole frame in LDS"),
    "MI355_FFT_WAVE_GEO": ("fft", "process", "alternative", "one-wave workgroups for N <= 1024"),
    "MI355_FFT_NO_TILE": ("fft", "create", "alternative", "decimation-in-time passes for 65536 ... 2^20 points"),
    "MI355_FFT_32768_TWO_KERNELS": ("fft", "create", "alternative", "32768 points through the workspace scheme"),
    "MI355_FFT_32768_IN_REGISTERS": ("fft", "call", "alternative", "32768 points in the registers of 256 threads"),
    "MI355_FFT_TILE_HALF": ("fft", "process", "alternative", "1024-row tile passes without the half-thread form"),
    "MI355_FFT_TILE_N1": ("fft", "create", "tuning", "row count of the first tile pass"),
    "MI355_FFT_TILE_WREG": ("fft", "call", "tuning", "window values of the first tile pass per item / in registers"),
    "MI355_FFT_WS_MB": ("fft", "process", "tuning", "workspace bound of the multi-pass sizes: several pieces per call"),
    "MI355_FFT_PREFETCH": ("fft", "call", "reroute", "prefetching / plain / two-groups-of-lead form of k_fft"),
    "MI355_FFT_SCHED": ("fft", "call", "identical", "dynamic claims or static stride of the persistent FFT"),
    "MI355_FFT_WG_PER_CU": ("fft", "call", "tuning", "grid of k_fft"),
    "MI355_FFT_NO_MR": ("fft", "create", "reroute", "2-3-5-7-11-13 lengths through chirp-z"),
    "MI355_FFT_MR_VARIANT": ("fft", "create", "reroute", "pins the mixed-radix factorisation"),
    "MI355_FFT_MR_TIMED_VARIANT": ("fft", "create", "tuning", "factorisation by a timing at the first handle of a length"),
    "MI355_FFT_MR_AUTOTUNE": ("fft", "create", "tuning", "workgroup size and frames per iteration by rule"),
    "MI355_FFT_MR_THREADS": ("fft", "create", "tuning", "forced workgroup size of k_fft_mr"),
    "MI355_FFT_MR_FRAMES": ("fft", "create", "tuning", "forced frames per iteration of k_fft_mr"),
    "MI355_FFT_MR_NO_COPY_OUT": ("fft", "process", "alternative", "k_fft_mr with the passes' own loads and stores"),
    "MI355_FFT_MR_COPY_OUT_NS": ("fft", "process", "alternative", "run length below which k_fft_mr stores through LDS"),
    "MI355_FFT_MR_COPY_IN_NB": ("fft", "process", "alternative", "run length below which k_fft_mr loads through LDS"),
    "MI355_FFT_TS": ("fft", "call", "not_run", "timestamp dump of the persistent FFT (a synchronous measuring launch)"),
    "MI355_FFT_TS_FILE": ("fft", "call", "not_run", "file the timestamp dump goes to"),
    # ---------------------------------------------------------------------------------------------------------------- filters
    "MI355_FIR_MFMA": ("filter", "process", "alternative", "k_fir_td with 16 or more taps"),
    "MI355_FIR_DEC_LDS_OFF": ("filter", "call", "alternative", "no LDS-staged decimator"),
    "MI355_FIR_DEC_LDS_MIN": ("filter", "process", "tuning", "smallest decimation of the LDS-staged kernels"),
    "MI355_FIR_DEC2_OFF": ("filter", "call", "reroute", "k_fir_dec_lds instead of k_fir_dec2"),
    "MI355_FIR_DEC2_EVEN_ONLY": ("filter", "call", "alternative", "k_fir_dec2 for even decimations only"),
    "MI355_FIR_DEC2_FROM_6": ("filter", "call", "alternative", "decimations 3 ... 5 on the every-output kernels"),
    "MI355_FIR_DEC2_SPAN": ("filter", "process", "tuning", "samples per tile of k_fir_dec2"),
    "MI355_FIR_DEC2_PAD": ("filter", "call", "tuning", "LDS padding shift of k_fir_dec2"),
    "MI355_FIR_DEC_KERNEL": ("filter", "call", "reroute", "forces one of the three decimating kernels"),
    "MI355_TD_WG_PER_CU": ("filter", "call", "tuning", "grid of the direct-form kernels"),
    "MI355_FILTER_FFT": ("filter", "create", "reroute", "transform size of the fast-convolution filter"),
    "MI355_FILTER_WAVE_GEO": ("filter", "call", "reroute", "four-wave / one-wave workgroups of k_ols"),
    "MI355_OLS_ALIGN": ("filter", "process", "alternative", "blocks that start storing at ntaps - 1"),
    "MI355_OLS_RAGGED_L": ("filter", "call", "alternative", "block length that is no multiple of 16"),
    "MI355_OLS_XCD_MAP": ("filter", "call", "alternative", "XCD-contiguous groups of k_ols"),
    "MI355_OLS_PART_XCD_MAP": ("filter", "call", "alternative", "k_ols_part with its groups in plain order"),
    "MI355_OLS_PART_ONE_PASS": ("filter", "process", "alternative", "segment loop of k_ols for partitioned filters"),
    "MI355_OLS_UPS": ("filter", "call", "reroute", "general partitioned kernel for 2049 ... 10240 taps"),
    "MI355_OLS_UPS_WGS": ("filter", "call", "tuning", "workgroups of k_ols_ups"),
    # ------------------------------------------------------------------------------------------------------------ channelizer
    "MI355_PFB_WAVE": ("pfb", "process", "alternative", "staged kernel for every channel count (512 channels: the two-kernel form)"),
    "MI355_PFB_SMALL": ("pfb", "call", "reroute", "ring kernel for calls of few groups"),
    "MI355_PFB_WAVES_PER_CU": ("pfb", "call", "tuning", "grid of the ring kernel"),
    "MI355_PFB_NO_RING_512": ("pfb", "create", "alternative", "512 channels through branch filters + clFFT"),
    "MI355_PFB_NO_XCD_RUNS": ("pfb", "process", "alternative", "k_pfb_branches_t with its workgroups in plain order"),
    "MI355_PFB_NO_FIR_RING": ("pfb", "call", "reroute", "k_pfb_branches_t instead of k_pfb_fir"),
    "MI355_PFB_NO_FAST_OVERSAMPLED": ("pfb", "create", "reroute", "oversampled geometries through the two-kernel form"),
    "MI355_PFB_NO_MR_FUSED": ("pfb", "call", "reroute", "two kernels instead of k_pfb_mr"),
    "MI355_PFB_DIRECT_DFT": ("pfb", "create", "reroute", "M products per output instead of the clFFT transform"),
    "MI355_PFB_BRANCHES_PER_OUTPUT": ("pfb", "call", "reroute", "one thread per branch output"),
    "MI355_PFB_MR_THREADS": ("pfb", "process", "tuning", "workgroup size of k_pfb_mr"),
    "MI355_PFB_MR_WG_PER_CU": ("pfb", "process", "tuning", "workgroups per CU of k_pfb_mr"),
    "MI355_PFB_MR_DBG": ("pfb", "call", "not_run", "phase elimination of k_pfb_mr: wrong results by design"),
    # ------------------------------------------------------------------------------------- resampler, synthesizer, loops
    "MI355_RESAMPLER_PLAIN": ("resampler", "create", "alternative", "k_rs_plain for every handle"),
    "MI355_RESAMPLER_GENERAL": ("resampler", "create", "reroute", "k_rs_lds where k_rs_interp would serve"),
    "MI355_SYNTH_TAPS_GLOBAL": ("synth", "create", "alternative", "taps through the caches although they fit the LDS"),
    "MI355_SYNTH_GENERIC": ("synth", "create", "reroute", "the generic route"),
    "MI355_SIGSOURCE_LITERAL": ("loops", "create", "reroute", "one sincos per item for complex / float output too"),
    "MI355_COSTAS_ONE_LANE": ("loops", "create", "reroute", "one stream as one lane of the several-streams kernel"),
    # --------------------------------------------------------------------------------------------------------------- X-engine
    "MI355_XE_NO_FUSED": ("xengine", "call", "alternative", "corner turn + correlator for <= 64 rows"),
    "MI355_XE_NO_LDS": ("xengine", "call", "alternative", "k_xe_corr, the correlator without LDS staging"),
    "MI355_XE_SLOW_TURN": ("xengine", "call", "alternative", "generic corner turn for whole-line rows"),
    "MI355_XE_SLABS": ("xengine", "call", "alternative", "several channel slabs through one workspace"),
    "MI355_XE_NO_SB": ("xengine", "call", "alternative", "65 ... 256 rows through k_xe_corr_lds / k_xe_corr"),
    "MI355_XE_NO_SB8": ("xengine", "call", "alternative", "65 ... 128 rows through k_xe_corr_lds"),
    "MI355_XE_CF32_VALU": ("xengine", "call", "reroute", "complex float on the vector ALU"),
    "MI355_XE_CF32_TWO_KERNELS": ("xengine", "call", "alternative", "complex float, <= 64 rows: corner turn + correlator"),
    "MI355_XE_CF32_CH": ("xengine", "call", "alternative", "four channels per workgroup of k_xe_f32_fused"),
    "MI355_XE_CF32_TSPLIT": ("xengine", "call", "alternative", "forced time ranges of k_xe_f32_fused"),
    "MI355_XE_CF32_PAD_COPY": ("xengine", "call", "reroute", "ragged complex-float rows through a padded copy"),
    "MI355_XE_CF32_NO_PAD": ("xengine", "create", "reroute", "ragged complex-float rows on the vector ALU"),
    "MI355_XE_FUSED_WHOLE_LINES": ("xengine", "call", "alternative", "rows that end inside a line through the two-kernel path"),
    "MI355_XE_FUSED_WHOLE_KBLOCKS": ("xengine", "call", "alternative", "ragged integrations through the two-kernel path"),
    "MI355_XE_TSPLIT": ("xengine", "call", "reroute", "time ranges of the fused kernel"),
    "MI355_XE_INKERNEL_REDUCE": ("xengine", "call", "reroute", "time ranges combined inside / after the launch"),
    "MI355_XE_NO_COMPACT": ("xengine", "call", "identical", "two records per diagonal tile pair"),
    "MI355_XE_NO_PACK24": ("xengine", "call", "identical", "32-bit partial sums"),
    "MI355_XE_NO_PINGPONG": ("xengine", "call", "identical", "fused kernel without the ping-pong schedule"),
    "MI355_XE_SCALE_F64": ("xengine", "call", "identical", "IChar scale in double"),
    "MI355_XE_REDUCE_IPW": ("xengine", "call", "tuning", "items per wave of k_xe_i8_reduce"),
    "MI355_XE_WAIT_US": ("xengine", "call", "tuning", "bounded wait of the in-launch reduction"),
    "MI355_XE_NO_PREFETCH": ("xengine", "call", "identical", "no early touches of the slow lines"),
    "MI355_XE_PF": ("xengine", "call", "tuning", "distance of the early touches"),
    "MI355_XE_SLOW_FIRST": ("xengine", "call", "identical", "slow lines' units first"),
    "MI355_XE_NO_SLOW_FIRST": ("xengine", "call", "identical", "slow lines' units in plain order"),
    "MI355_XE_NO_PERSIST": ("xengine", "call", "identical", "one unit per workgroup"),
    "MI355_XE_NO_SPLIT": ("xengine", "call", "identical", "one launch for a window count the whole-line kernel does not take"),
    "MI355_XE_NO_LINES": ("xengine", "call", "reroute", "never the whole-line kernel"),
    "MI355_XE_NO_LINES2": ("xengine", "call", "reroute", "two polarisations through corner turn + correlator"),
    "MI355_XE_NO_LINES_SPLIT": ("xengine", "call", "reroute", "one / two windows through the 32-byte-slice kernel"),
    "MI355_XE_LINES_SPLIT_ANY": ("xengine", "call", "reroute", "time-range form of the whole-line kernel for any unit count"),
    "MI355_XE_LINES_MIN_UNITS": ("xengine", "call", "reroute", "whole-line kernel for any unit count"),
    "MI355_XE_LINES_MAX_ITEMS": ("xengine", "call", "reroute", "largest share of units per workgroup the whole-line kernel takes"),
    "MI355_XE_LINES_ROT": ("xengine", "call", "identical", "rotation of a workgroup's later units over the lines"),
    "MI355_XE_LINES_PUB": ("xengine", "call", "identical", "progress words published at agent scope"),
    "MI355_XE_LINES_PF": ("xengine", "call", "identical", "early touches of the whole-line kernel"),
    "MI355_XE_LINES_PACE": ("xengine", "call", "identical", "pacing of a line's four workgroups"),
    "MI355_XE_DBG": ("xengine", "call", "not_run", "phase elimination: wrong results by design"),
    "MI355_XE_FAIL_LAUNCH": ("xengine", "call", "not_run", "makes the launch fail: used by tests/test_xengine_gpu.py for the recovery paths"),
    "MI355_XE_TS": ("xengine", "call", "not_run", "timestamp dump (a synchronous measuring launch)"),
    "MI355_XE_TS_FILE": ("xengine", "call", "not_run", "file the timestamp dump goes to"),
}

_READ = re.compile(r'(?:getenv|env_set)\("(MI355_[A-Z0-9_]+)"')


def source_reads():
    """[(file, line number, line text, name)] for every getenv / env_set of an MI355_* name under csrc/"""
    out = []
    for fn in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, fn)
        if not os.path.isfile(path):
            continue
        with open(path, encoding="utf-8", errors="replace") as f:
            for no, line in enumerate(f, 1):
                for name in _READ.findall(line):
                    out.append((fn, no, line, name))
    return out


def source_names():
    return {r[3] for r in source_reads()}


def static_names():
    """names read in a `static` initialiser on the same line: once per process"""
    return {name for _, _, line, name in source_reads() if re.search(r"\bstatic\b", line)}


# names INTEGRATION.md's table documents that are not this library's to read: the C++ host layer's (gr-clenabled_amd/host/)
HOST_LAYER = {"MI355_XENGINE_SHARD_WINDOWS", "MI355_XENGINE_DEVICES"}


def doc_names():
    """names in the first column of INTEGRATION.md's table of environment switches"""
    names = set()
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        for line in f:
            if line.startswith("| `MI355_"):
                names.update(re.findall(r"`(MI355_[A-Z0-9_]+)`", line.split("|")[1]))
    return names
