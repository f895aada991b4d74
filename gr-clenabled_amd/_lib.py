"""Loader for libmi355_clenabled.so (the C ABI in include/mi355_clenabled.h).

There is no fallback of any kind: if the shared library is missing or a call
fails, an exception is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355_clenabled.so")
_lib = None


class Mi355Error(RuntimeError):
    def __init__(self, code, where, detail):
        super().__init__("%s failed: %s (%d) %s" % (where, _strerror(code), code, detail))
        self.code = code


def _strerror(code):
    try:
        return lib().mi355_strerror(code).decode()
    except Exception:  # pragma: no cover
        return "?"


LOG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)  # mi355_log_fn
_log_keepalive = None


def set_log_callback(fn):
    """fn(level, message) receives every diagnostics / error line of the library (None restores stderr)."""
    global _log_keepalive
    cb = LOG_FN(lambda user, level, msg: fn(level, msg.decode())) if fn is not None else C.cast(None, LOG_FN)
    check(lib().mi355_set_log_callback(cb, None), "mi355_set_log_callback")
    _log_keepalive = cb  # the C side holds the pointer: keep the thunk alive


def lib():
    """Return the ctypes handle, loading the library on first use."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `make -C %s/csrc` (or __graft_entry__.build()); "
            "gr-clenabled_amd has no non-HIP fallback" % (LIB_PATH, _HERE))
    try:
        # torch ships its own libamdhip64 (same SONAME); importing it first makes
        # this library bind to the HIP runtime that owns torch's device memory.
        import torch  # noqa: F401
    except Exception:  # torch is plumbing, not a requirement of the C ABI
        pass
    L = C.CDLL(LIB_PATH)
    vp, i, sz, f = C.c_void_p, C.c_int, C.c_size_t, C.c_float
    pp = C.POINTER(C.c_void_p)
    d, dp = C.c_double, C.POINTER(C.c_double)
    ll, llp = C.c_longlong, C.POINTER(C.c_longlong)
    sigs = {
        "mi355_strerror": (C.c_char_p, [i]),
        "mi355_last_error": (C.c_char_p, []),
        "mi355_version": (C.c_char_p, []),
        "mi355_set_log_callback": (i, [LOG_FN, vp]),
        "mi355_device_count": (i, []),
        "mi355_ctx_create": (i, [i, i, i, i, i, pp]),
        "mi355_ctx_destroy": (i, [vp]),
        "mi355_ctx_device": (i, [vp]),
        "mi355_ctx_stream": (vp, [vp]),
        "mi355_ctx_synchronize": (i, [vp]),
        "mi355_malloc": (i, [vp, sz, pp]),
        "mi355_free": (i, [vp, vp]),
        "mi355_memcpy_h2d": (i, [vp, vp, vp, sz]),
        "mi355_memcpy_d2h": (i, [vp, vp, vp, sz]),
        "mi355_mathop_create": (i, [vp, i, i, sz, pp]),
        "mi355_mathop_destroy": (i, [vp]),
        "mi355_mathop_work": (i, [vp, sz, vp, vp, vp]),
        "mi355_mathop_work_dev": (i, [vp, sz, vp, vp, vp, vp]),
        "mi355_mathconst_create": (i, [vp, i, i, f, sz, pp]),
        "mi355_mathconst_destroy": (i, [vp]),
        "mi355_mathconst_set_k": (i, [vp, f]),
        "mi355_mathconst_get_k": (i, [vp, C.POINTER(f)]),
        "mi355_mathconst_work": (i, [vp, sz, vp, vp]),
        "mi355_mathconst_work_dev": (i, [vp, sz, vp, vp, vp]),
        "mi355_fft_create": (i, [vp, i, i, vp, i, i, i, i, pp]),
        "mi355_fft_destroy": (i, [vp]),
        "mi355_fft_plan_text": (i, [i, C.c_char_p, i]),
        "mi355_fft_last_route": (C.c_char_p, [vp]),
        "mi355_fft_work": (i, [vp, i, pp, pp]),
        "mi355_fft_work_dev": (i, [vp, i, vp, vp, vp]),
        "mi355_filter_create": (i, [vp, i, vp, i, i, i, pp]),
        "mi355_filter_destroy": (i, [vp]),
        "mi355_filter_set_taps": (i, [vp, vp, i]),
        "mi355_filter_ntaps": (i, [vp]),
        "mi355_filter_get_taps": (i, [vp, vp, i]),
        "mi355_filter_fftsize": (i, [vp]),
        "mi355_filter_work": (i, [vp, sz, vp, vp]),
        "mi355_filter_work_dev": (i, [vp, sz, vp, vp, vp]),
        "mi355_filter_last_route": (C.c_char_p, [vp]),
        "mi355_pfb_create": (i, [vp, vp, i, i, i, i, vp, i, pp]),
        "mi355_pfb_destroy": (i, [vp]),
        "mi355_pfb_noutput": (i, [vp]),
        "mi355_pfb_ninput": (i, [vp]),
        "mi355_pfb_work": (i, [vp, vp, vp]),
        "mi355_pfb_work_dev": (i, [vp, vp, vp, vp]),
        "mi355_pfb_work_dev_n": (i, [vp, i, vp, vp, vp]),
        "mi355_pfb_last_route": (C.c_char_p, [vp]),
        "mi355_xengine_create": (i, [vp, i, i, i, i, i, pp]),
        "mi355_xengine_destroy": (i, [vp]),
        "mi355_xengine_input_bytes": (sz, [vp]),
        "mi355_xengine_output_items": (sz, [vp]),
        "mi355_xengine_xcorrelate": (i, [vp, vp, vp, i]),
        "mi355_xengine_xcorrelate_dev": (i, [vp, vp, vp, i, vp]),
        "mi355_xengine_xcorrelate_grouped_dev": (i, [vp, vp, vp, i, i, vp]),
        "mi355_xengine_xcorrelate_n_dev": (i, [vp, i, vp, vp, i, i, vp]),
        "mi355_pack3d_dev": (i, [vp, vp, vp, sz, sz, sz, sz, sz, sz, sz, vp]),
        "mi355_xengine_gather": (i, [vp, i, i, pp, vp]),
        "mi355_xengine_selftest_scale": (i, [vp, C.POINTER(C.c_longlong)]),
        "mi355_xengine_last_route": (i, [vp, vp]),
        "mi355_xengine_shard_create": (i, [i, C.POINTER(C.c_int), i, i, i, i, i, pp]),
        "mi355_xengine_shard_destroy": (i, [vp]),
        "mi355_xengine_shard_world": (i, [vp]),
        "mi355_xengine_shard_device": (i, [vp, i]),
        "mi355_xengine_shard_frames_bytes": (sz, [vp]),
        "mi355_xengine_shard_slab_items": (sz, [vp]),
        "mi355_xengine_shard_stream": (vp, [vp, i]),
        "mi355_xengine_shard_submit_dev": (i, [vp, pp, pp, i]),
        "mi355_xengine_shard_wait_stream": (i, [vp, i, vp]),
        "mi355_xengine_shard_synchronize": (i, [vp]),
        "mi355_xengine_shard_xcorrelate": (i, [vp, vp, vp, i]),
        "mi355_xengine_shard_windows": (i, [vp]),
        "mi355_xengine_shard_input_bytes": (sz, [vp]),
        "mi355_xengine_shard_acquire": (i, [vp, pp]),
        "mi355_xengine_shard_submit_acquired": (i, [vp]),
        "mi355_xengine_shard_wait": (i, [vp, vp]),
        "mi355_xengine_shard_pending": (i, [vp]),
        "mi355_xengine_submit": (i, [vp, vp, vp]),
        "mi355_xengine_wait": (i, [vp, vp]),
        "mi355_xengine_pending": (i, [vp]),
        "mi355_xengine_acquire": (i, [vp, pp]),
        "mi355_xengine_submit_acquired": (i, [vp, vp]),
        "mi355_elem_create": (i, [vp, i, f, f, pp]),
        "mi355_elem_destroy": (i, [vp]),
        "mi355_elem_history": (i, [vp]),
        "mi355_elem_work": (i, [vp, sz, vp, vp, vp, vp]),
        "mi355_elem_work_dev": (i, [vp, sz, vp, vp, vp, vp, vp]),
        "mi355_xcorr_fft_create": (i, [vp, i, i, i, pp]),
        "mi355_xcorr_fft_destroy": (i, [vp]),
        "mi355_xcorr_fft_work": (i, [vp, i, vp, vp]),
        "mi355_xcorr_fft_work_dev": (i, [vp, i, vp, vp, vp]),
        "mi355_xcorr_td_plan": (i, [i, i, C.POINTER(C.c_int)]),
        "mi355_xcorr_td_create": (i, [vp, i, i, i, i, i, pp]),
        "mi355_xcorr_td_destroy": (i, [vp]),
        "mi355_xcorr_td_max_shift": (i, [vp]),
        "mi355_xcorr_td_work": (i, [vp, pp, vp, vp]),
        "mi355_xcorr_td_submit": (i, [vp, pp]),
        "mi355_xcorr_td_poll": (i, [vp, vp, vp]),
        "mi355_xcorr_td_wait": (i, [vp]),
        "mi355_xcorr_td_work_dev": (i, [vp, i, pp, vp, vp, vp, vp]),
        "mi355_sigsource_create": (i, [vp, i, d, i, d, f, pp]),
        "mi355_sigsource_destroy": (i, [vp]),
        "mi355_sigsource_set_frequency": (i, [vp, d]),
        "mi355_sigsource_get_state": (i, [vp, dp, dp]),
        "mi355_sigsource_set_phase": (i, [vp, d]),
        "mi355_sigsource_work": (i, [vp, sz, vp]),
        "mi355_sigsource_work_dev": (i, [vp, sz, vp, vp]),
        "mi355_costas_plan": (i, [f, i, C.POINTER(f), C.POINTER(f)]),
        "mi355_costas_create": (i, [vp, f, i, i, pp]),
        "mi355_costas_destroy": (i, [vp]),
        "mi355_costas_set_loop_bandwidth": (i, [vp, f]),
        "mi355_costas_get_state": (i, [vp, vp, vp, vp]),
        "mi355_costas_set_state": (i, [vp, vp, vp]),
        "mi355_costas_work": (i, [vp, sz, vp, vp, vp]),
        "mi355_costas_work_dev": (i, [vp, sz, vp, vp, vp, vp]),
        "mi355_resampler_plan": (i, [i, i, i, i, ll, C.POINTER(i), llp, llp, C.POINTER(i)]),
        "mi355_resampler_noutput_for": (ll, [i, i, i, i, ll]),
        "mi355_resampler_create": (i, [vp, i, i, vp, i, i, pp]),
        "mi355_resampler_destroy": (i, [vp]),
        "mi355_resampler_set_taps": (i, [vp, vp, i]),
        "mi355_resampler_ntaps": (i, [vp]),
        "mi355_resampler_get_taps": (i, [vp, vp, i]),
        "mi355_resampler_history": (i, [vp]),
        "mi355_resampler_get_phase": (i, [vp, C.POINTER(i)]),
        "mi355_resampler_set_phase": (i, [vp, i]),
        "mi355_resampler_work": (i, [vp, ll, vp, vp, llp]),
        "mi355_resampler_work_dev": (i, [vp, ll, vp, vp, llp, vp]),
        "mi355_synth_plan": (i, [i, i, i, ll, C.POINTER(i), llp, llp]),
        "mi355_synth_create": (i, [vp, vp, i, i, vp, i, pp]),
        "mi355_synth_destroy": (i, [vp]),
        "mi355_synth_set_taps": (i, [vp, vp, i]),
        "mi355_synth_ntaps": (i, [vp]),
        "mi355_synth_get_taps": (i, [vp, vp, i]),
        "mi355_synth_taps_per_arm": (i, [vp]),
        "mi355_synth_num_channels": (i, [vp]),
        "mi355_synth_nmap": (i, [vp]),
        "mi355_synth_route": (C.c_char_p, [vp]),
        "mi355_synth_work": (i, [vp, ll, vp, vp]),
        "mi355_synth_work_dev": (i, [vp, ll, vp, vp, vp]),
        "mi355_pspec_plan": (i, [i, i, i, ll, llp, llp]),
        "mi355_pspec_create": (i, [vp, i, vp, i, i, i, i, i, f, pp]),
        "mi355_pspec_destroy": (i, [vp]),
        "mi355_pspec_set_scale": (i, [vp, f]),
        "mi355_pspec_set_window": (i, [vp, vp, i]),
        "mi355_pspec_set_generic": (i, [vp, i]),
        "mi355_pspec_fft_size": (i, [vp]),
        "mi355_pspec_navg": (i, [vp]),
        "mi355_pspec_hop": (i, [vp]),
        "mi355_pspec_route": (C.c_char_p, [vp]),
        "mi355_pspec_work": (i, [vp, ll, vp, vp]),
        "mi355_pspec_work_dev": (i, [vp, ll, vp, vp, vp]),
        "mi355_xlate_plan": (i, [i, i, ll, llp, C.POINTER(i)]),
        "mi355_xlate_create": (i, [vp, i, vp, i, i, d, dp, i, i, pp]),
        "mi355_xlate_destroy": (i, [vp]),
        "mi355_xlate_set_taps": (i, [vp, vp, i]),
        "mi355_xlate_ntaps": (i, [vp]),
        "mi355_xlate_get_taps": (i, [vp, vp, i]),
        "mi355_xlate_num_channels": (i, [vp]),
        "mi355_xlate_decimation": (i, [vp]),
        "mi355_xlate_set_center_freq": (i, [vp, i, d]),
        "mi355_xlate_get_center_freq": (i, [vp, i, dp]),
        "mi355_xlate_get_bandpass_taps": (i, [vp, i, vp, i]),
        "mi355_xlate_get_state": (i, [vp, i, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
        "mi355_xlate_set_phase": (i, [vp, i, C.c_ulonglong]),
        "mi355_xlate_skip": (i, [vp, ll]),
        "mi355_xlate_set_generic": (i, [vp, i]),
        "mi355_xlate_route": (C.c_char_p, [vp]),
        "mi355_xlate_work": (i, [vp, ll, vp, pp]),
        "mi355_xlate_work_dev": (i, [vp, ll, vp, pp, vp]),
        "mi355_beamform_plan": (i, [i, i, i, i, i, i, i, llp, C.POINTER(i), llp]),
        "mi355_beamform_create": (i, [vp, i, i, i, i, i, i, i, vp, pp]),
        "mi355_beamform_destroy": (i, [vp]),
        "mi355_beamform_set_weights": (i, [vp, vp]),
        "mi355_beamform_set_beam_weights": (i, [vp, i, vp]),
        "mi355_beamform_get_weights": (i, [vp, vp, ll]),
        "mi355_beamform_num_beams": (i, [vp]),
        "mi355_beamform_frame_bytes": (ll, [vp]),
        "mi355_beamform_out_bytes_per_unit": (ll, [vp]),
        "mi355_beamform_set_generic": (i, [vp, i]),
        "mi355_beamform_route": (C.c_char_p, [vp]),
        "mi355_beamform_work": (i, [vp, ll, vp, vp]),
        "mi355_beamform_work_dev": (i, [vp, ll, vp, vp, vp]),
        "mi355_fengine_plan": (i, [i, i, i, i, i, ll, llp, llp, llp]),
        "mi355_fengine_create": (i, [vp, i, i, i, i, vp, i, vp, pp]),
        "mi355_fengine_destroy": (i, [vp]),
        "mi355_fengine_set_gains": (i, [vp, vp]),
        "mi355_fengine_set_input_gain": (i, [vp, i, vp]),
        "mi355_fengine_get_gains": (i, [vp, vp, ll]),
        "mi355_fengine_get_clips": (i, [vp, vp, i]),
        "mi355_fengine_set_generic": (i, [vp, i]),
        "mi355_fengine_route": (C.c_char_p, [vp]),
        "mi355_fengine_frame_bytes": (ll, [vp]),
        "mi355_fengine_history_items": (ll, [vp]),
        "mi355_fengine_work": (i, [vp, ll, pp, vp]),
        "mi355_fengine_work_dev": (i, [vp, ll, pp, vp, vp]),
        "mi355_dedisp_plan": (i, [i, i, i, i, i, llp, llp, llp]),
        "mi355_dedisp_create": (i, [vp, i, i, i, i, i, vp, pp]),
        "mi355_dedisp_destroy": (i, [vp]),
        "mi355_dedisp_set_delays": (i, [vp, vp]),
        "mi355_dedisp_get_delays": (i, [vp, vp, ll]),
        "mi355_dedisp_history": (ll, [vp]),
        "mi355_dedisp_set_generic": (i, [vp, i]),
        "mi355_dedisp_route": (C.c_char_p, [vp]),
        "mi355_dedisp_work": (i, [vp, ll, vp, vp, ll]),
        "mi355_dedisp_work_dev": (i, [vp, ll, vp, vp, ll, vp]),
        "mi355_dedisp_delays": (i, [d, d, i, d, vp, i, vp, C.POINTER(i)]),
        "mi355_psearch_plan": (i, [i, i, i, i, i, llp, llp, llp]),
        "mi355_psearch_create": (i, [vp, i, i, i, i, i, vp, vp, pp]),
        "mi355_psearch_destroy": (i, [vp]),
        "mi355_psearch_set_stats": (i, [vp, vp, vp]),
        "mi355_psearch_get_stats": (i, [vp, vp, vp, ll]),
        "mi355_psearch_set_threshold": (i, [vp, f]),
        "mi355_psearch_history": (ll, [vp]),
        "mi355_psearch_set_generic": (i, [vp, i]),
        "mi355_psearch_route": (C.c_char_p, [vp]),
        "mi355_psearch_work": (i, [vp, ll, vp, ll, vp, vp, ll, vp]),
        "mi355_psearch_work_dev": (i, [vp, ll, vp, ll, vp, vp, ll, vp, vp]),
        "mi355_psearch_measure": (i, [vp, ll, vp, ll, i, vp, vp]),
        "mi355_fbclean_plan": (i, [i, i, i, llp, llp, llp]),
        "mi355_fbclean_create": (i, [vp, i, i, i, d, d, d, d, i, vp, pp]),
        "mi355_fbclean_destroy": (i, [vp]),
        "mi355_fbclean_set_limits": (i, [vp, d, d, d, d, i]),
        "mi355_fbclean_get_limits": (i, [vp, dp, dp, dp, dp, C.POINTER(i)]),
        "mi355_fbclean_set_mask": (i, [vp, vp]),
        "mi355_fbclean_get_mask": (i, [vp, vp, ll]),
        "mi355_fbclean_block_len": (ll, [vp]),
        "mi355_fbclean_set_generic": (i, [vp, i]),
        "mi355_fbclean_route": (C.c_char_p, [vp]),
        "mi355_fbclean_work": (i, [vp, ll, vp, vp, vp, vp, vp]),
        "mi355_fbclean_work_dev": (i, [vp, ll, vp, vp, vp, vp, vp, vp]),
        "mi355_fbclean_sk_estimate": (i, [vp, i, ll, d, dp]),
        "mi355_fold_plan": (i, [i, i, i, i, llp, llp, llp]),
        "mi355_fold_create": (i, [vp, i, i, i, i, vp, pp]),
        "mi355_fold_destroy": (i, [vp]),
        "mi355_fold_set_models": (i, [vp, vp]),
        "mi355_fold_get_models": (i, [vp, vp, ll]),
        "mi355_fold_sample": (i, [vp, C.POINTER(C.c_ulonglong)]),
        "mi355_fold_set_sample": (i, [vp, C.c_ulonglong]),
        "mi355_fold_skip": (i, [vp, ll]),
        "mi355_fold_subint_len": (ll, [vp]),
        "mi355_fold_set_generic": (i, [vp, i]),
        "mi355_fold_route": (C.c_char_p, [vp]),
        "mi355_fold_work": (i, [vp, ll, vp, vp, vp, vp]),
        "mi355_fold_work_dev": (i, [vp, ll, vp, vp, vp, vp, vp]),
        "mi355_fold_model": (i, [d, d, d, d, vp]),
        "mi355_fold_bins": (i, [vp, C.c_ulonglong, ll, i, vp]),
        "mi355_ffa_plan": (i, [i, i, i, i, i, llp, llp, llp, llp]),
        "mi355_ffa_create": (i, [vp, i, i, i, i, i, vp, vp, pp]),
        "mi355_ffa_destroy": (i, [vp]),
        "mi355_ffa_set_stats": (i, [vp, vp, vp]),
        "mi355_ffa_get_stats": (i, [vp, vp, vp, ll]),
        "mi355_ffa_set_generic": (i, [vp, i]),
        "mi355_ffa_route": (C.c_char_p, [vp]),
        "mi355_ffa_work": (i, [vp, vp, ll, vp, vp]),
        "mi355_ffa_work_dev": (i, [vp, vp, ll, vp, vp, vp]),
        "mi355_ffa_shift": (ll, [i, i, i]),
        "mi355_ffa_period": (d, [i, i, i, d]),
        "mi355_ssearch_plan": (i, [i, i, i, i, i, i, llp, llp, llp]),
        "mi355_ssearch_create": (i, [vp, i, i, i, i, i, i, vp, pp]),
        "mi355_ssearch_destroy": (i, [vp]),
        "mi355_ssearch_set_stats": (i, [vp, vp]),
        "mi355_ssearch_get_stats": (i, [vp, vp, ll]),
        "mi355_ssearch_set_threshold": (i, [vp, f]),
        "mi355_ssearch_set_generic": (i, [vp, i]),
        "mi355_ssearch_route": (C.c_char_p, [vp]),
        "mi355_ssearch_fft_route": (C.c_char_p, [vp]),
        "mi355_ssearch_work": (i, [vp, vp, ll, vp, vp, vp, ll, vp]),
        "mi355_ssearch_work_dev": (i, [vp, vp, ll, vp, vp, vp, ll, vp, vp]),
        "mi355_ssearch_freq": (d, [i, d, i, i]),
        "mi355_accel_plan": (i, [i, i, i, llp, llp, llp]),
        "mi355_accel_create": (i, [vp, i, i, i, vp, pp]),
        "mi355_accel_destroy": (i, [vp]),
        "mi355_accel_set_trials": (i, [vp, vp]),
        "mi355_accel_get_trials": (i, [vp, vp, ll]),
        "mi355_accel_set_generic": (i, [vp, i]),
        "mi355_accel_route": (C.c_char_p, [vp]),
        "mi355_accel_work": (i, [vp, vp, ll, vp, ll, i, i]),
        "mi355_accel_work_dev": (i, [vp, vp, ll, vp, ll, i, i, vp]),
        "mi355_accel_coeff": (i, [i, d, d, llp]),
        "mi355_accel_index": (i, [i, ll, ll, ll, vp]),
        "mi355_accel_trials": (i, [i, d, d, d, d, vp, ll, llp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    L._declared = tuple(sigs)
    _lib = L
    return L


def check(code, where):
    if code != 0:
        raise Mi355Error(code, where, lib().mi355_last_error().decode())
    return code
