"""Host-side mirror of the gr::clenabled block API for the hot path.

Constructor arguments are the reference's ``make(...)`` arguments, in the same
positional order GRC passes them (include/clenabled/*.h, grc/*.block.yml), and
``work()/general_work()`` keep the ``noutput_items`` contract.  Everything is a
thin call into the C ABI (include/mi355_clenabled.h); there is no Python or CPU
compute path here.

Two flavours of each work call:
  work(noutput_items, input_items, output_items)         numpy (host) buffers,
      the GNU Radio contract: blocking, H2D / kernel / D2H inside the call
  work_device(noutput_items, input_items, output_items)  torch CUDA tensors,
      enqueue-only on torch's current stream (device-resident chaining / bench)
"""
import ctypes as C

import numpy as np

from ._lib import check, lib

# include/clenabled/GRCLBase.h:57-70, clMathOpTypes.h:11-20
DTYPE_COMPLEX, DTYPE_FLOAT, DTYPE_INT, DTYPE_SHORT, DTYPE_BYTE, DTYPE_PACKEDXY = 1, 2, 3, 4, 5, 6
OCLTYPE_GPU, OCLTYPE_ACCELERATOR, OCLTYPE_CPU, OCLTYPE_ANY = 1, 2, 3, 4
OCLDEVICESELECTOR_FIRST, OCLDEVICESELECTOR_SPECIFIC = 1, 2
MATHOP_MULTIPLY, MATHOP_ADD, MATHOP_SUBTRACT, MATHOP_COMPLEX_CONJUGATE, MATHOP_MULTIPLY_CONJUGATE = 1, 2, 3, 4, 5
MATHOP_EMPTY, MATHOP_EMPTY_W_COPY = 255, 254
CLFFT_FORWARD, CLFFT_BACKWARD = -1, 1
CLXCORR_TRIANGULAR_ORDER, CLXCORR_FULL_MATRIX = 1, 2

_NP_OF = {DTYPE_COMPLEX: np.complex64, DTYPE_FLOAT: np.float32, DTYPE_INT: np.int32}


def _host(a, dtype=None, writable=False):
    if not isinstance(a, np.ndarray) or not a.flags["C_CONTIGUOUS"] or (dtype is not None and a.dtype != dtype):
        if writable:
            raise TypeError("output buffers must be C-contiguous numpy arrays of dtype %s" % dtype)
        a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _hp(a):
    return C.c_void_p(a.ctypes.data)


def _dp(t, nbytes=None, name="device buffer"):
    """Device pointer of a contiguous CUDA tensor; nbytes: what the call reads or writes there (the C ABI takes plain pointers, so a
    tensor that is too short would be a memory fault on the device, not an error)."""
    if not t.is_cuda or not t.is_contiguous():
        raise TypeError("device path needs contiguous CUDA tensors")
    if nbytes is not None and t.numel() * t.element_size() < nbytes:
        raise ValueError("%s holds %d bytes, the call needs %d" % (name, t.numel() * t.element_size(), nbytes))
    return C.c_void_p(t.data_ptr())


def _torch_stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Block:
    """Owns one mi355 context, like every reference block owns one cl::Context
    (lib/GRCLBase.cpp:115-144)."""

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, setDebug):
        self._L = lib()
        self._ctx = C.c_void_p()
        self._h = C.c_void_p()
        check(self._L.mi355_ctx_create(int(openCLPlatformType), int(devSelector), int(platformId), int(devId),
                                       1 if setDebug else 0, C.byref(self._ctx)), "mi355_ctx_create")
        self.device = self._L.mi355_ctx_device(self._ctx)

    _destroy = None

    def stop(self):
        if getattr(self, "_h", None) and self._h.value and self._destroy:
            getattr(self._L, self._destroy)(self._h)
            self._h = C.c_void_p()
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.mi355_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()
        return True

    def __del__(self):
        try:
            self.stop()
        except Exception:
            pass

    def synchronize(self):
        check(self._L.mi355_ctx_synchronize(self._ctx), "mi355_ctx_synchronize")


def _need(name, arr, items):
    """work() contract: every buffer holds at least noutput_items items (the C ABI copies exactly that many)."""
    if arr.size < items:
        raise ValueError("%s holds %d items, the call needs %d" % (name, arr.size, items))


class clMathOp(_Block):
    """clMathOp::make(idataType, openCLPlatformType, devSelector, platformId, devId,
    operatorType, setDebug=0)  -- include/clenabled/clMathOp.h:42"""
    _destroy = "mi355_mathop_destroy"

    def __init__(self, idataType, openCLPlatformType, devSelector, platformId, devId, operatorType, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self.dtype = idataType
        check(self._L.mi355_mathop_create(self._ctx, int(idataType), int(operatorType), 0, C.byref(self._h)),
              "mi355_mathop_create")

    def work(self, noutput_items, input_items, output_items):
        dt = _NP_OF[self.dtype]
        if len(input_items) < 2 or len(output_items) < 1:
            raise ValueError("clMathOp.work needs two inputs and one output")
        a, b = _host(input_items[0], dt), _host(input_items[1], dt)
        c = _host(output_items[0], dt, writable=True)
        for name, arr in (("input 0", a), ("input 1", b), ("output", c)):
            _need(name, arr, noutput_items)
        check(self._L.mi355_mathop_work(self._h, noutput_items, _hp(a), _hp(b), _hp(c)), "mi355_mathop_work")
        return noutput_items

    testOpenCL = work  # lib/clMathOp_impl.cc:354-359

    def work_device(self, noutput_items, input_items, output_items):
        nb = int(noutput_items) * np.dtype(_NP_OF[self.dtype]).itemsize
        check(self._L.mi355_mathop_work_dev(self._h, noutput_items, _dp(input_items[0], nb, "input 0"), _dp(input_items[1], nb, "input 1"),
                                            _dp(output_items[0], nb, "output"), _torch_stream(self.device)), "mi355_mathop_work_dev")
        return noutput_items


class clMathConst(_Block):
    """clMathConst::make(idataType, openCLPlatformType, devSelector, platformId, devId,
    fValue, operatorType, setDebug=0)  -- include/clenabled/clMathConst.h:51"""
    _destroy = "mi355_mathconst_destroy"

    def __init__(self, idataType, openCLPlatformType, devSelector, platformId, devId, fValue, operatorType, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self.dtype = idataType
        check(self._L.mi355_mathconst_create(self._ctx, int(idataType), int(operatorType), float(fValue), 0,
                                             C.byref(self._h)), "mi355_mathconst_create")

    def k(self):
        v = C.c_float()
        check(self._L.mi355_mathconst_get_k(self._h, C.byref(v)), "mi355_mathconst_get_k")
        return v.value

    def set_k(self, newValue):
        check(self._L.mi355_mathconst_set_k(self._h, float(newValue)), "mi355_mathconst_set_k")

    def work(self, noutput_items, input_items, output_items):
        dt = _NP_OF[self.dtype]
        a = _host(input_items[0], dt)
        c = _host(output_items[0], dt, writable=True)
        _need("input", a, noutput_items)
        _need("output", c, noutput_items)
        check(self._L.mi355_mathconst_work(self._h, noutput_items, _hp(a), _hp(c)), "mi355_mathconst_work")
        return noutput_items

    testOpenCL = work

    def work_device(self, noutput_items, input_items, output_items):
        nb = int(noutput_items) * np.dtype(_NP_OF[self.dtype]).itemsize
        check(self._L.mi355_mathconst_work_dev(self._h, noutput_items, _dp(input_items[0], nb, "input"), _dp(output_items[0], nb, "output"),
                                               _torch_stream(self.device)), "mi355_mathconst_work_dev")
        return noutput_items


class clFFT(_Block):
    """clFFT::make(fftSize, clFFTDir, window, idataType, openCLPlatformType, devSelector,
    platformId, devId, setDebug=0, num_streams=1, shift=False) -- the positional
    order of lib/clFFT_impl.cc:34-36, which is what GRC emits
    (grc/clenabled_clFFT.block.yml:84-89); the header's parameter names differ
    (SURVEY App. B-1).  noutput_items counts VECTORS of fftSize items."""
    _destroy = "mi355_fft_destroy"

    def __init__(self, fftSize, clFFTDir, window, idataType, openCLPlatformType, devSelector, platformId, devId,
                 setDebug=0, num_streams=1, shift=False):
        window = np.ascontiguousarray(window if window is not None else [], dtype=np.float32)
        if not (window.size == 0 or window.size == fftSize):
            # lib/clFFT_impl.cc:74-76
            raise RuntimeError("OpenCL FFT: window not the same length as fft_size")
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self.fft_size, self.dtype, self.num_streams = int(fftSize), idataType, int(num_streams)
        check(self._L.mi355_fft_create(self._ctx, int(fftSize), int(clFFTDir), _hp(window) if window.size else None,
                                       int(window.size), int(idataType), int(num_streams), 1 if shift else 0,
                                       C.byref(self._h)), "mi355_fft_create")

    def work(self, noutput_items, input_items, output_items):
        dt = _NP_OF[self.dtype]
        if len(input_items) < self.num_streams or len(output_items) < self.num_streams:
            raise ValueError("clFFT.work needs %d input and output streams" % self.num_streams)
        ins = [_host(x, dt) for x in input_items[:self.num_streams]]
        outs = [_host(x, np.complex64, writable=True) for x in output_items[:self.num_streams]]
        for i, (x, y) in enumerate(zip(ins, outs)):
            _need("input %d" % i, x, noutput_items * self.fft_size)
            _need("output %d" % i, y, noutput_items * self.fft_size)
        pi = (C.c_void_p * len(ins))(*[x.ctypes.data for x in ins])
        po = (C.c_void_p * len(outs))(*[x.ctypes.data for x in outs])
        check(self._L.mi355_fft_work(self._h, noutput_items, pi, po), "mi355_fft_work")
        return noutput_items

    def testOpenCL(self, noutput_items, input_items, output_items):
        # the reference's test hook counts SAMPLES (lib/clFFT_impl.cc:520-524)
        return self.work(noutput_items // self.fft_size, input_items, output_items) * self.fft_size

    def work_device(self, noutput_items, input_items, output_items):
        st = _torch_stream(self.device)
        n = int(noutput_items) * self.fft_size
        for x, y in zip(input_items[:self.num_streams], output_items[:self.num_streams]):
            check(self._L.mi355_fft_work_dev(self._h, noutput_items, _dp(x, n * np.dtype(_NP_OF[self.dtype]).itemsize, "input"),
                                             _dp(y, n * 8, "output"), st), "mi355_fft_work_dev")
        return noutput_items

    def last_route(self):
        """The kernels the last work() / work_device() launched and their parameters (mi355_fft_last_route); "" before the first call."""
        return self._L.mi355_fft_last_route(self._h).decode()


class _FilterBase(_Block):
    _destroy = "mi355_filter_destroy"

    def _create(self, decimation, taps, complex_taps, use_time):
        self._complex = complex_taps
        self.decimation = int(decimation)
        t = np.ascontiguousarray(taps, dtype=np.complex64 if complex_taps else np.float32)
        check(self._L.mi355_filter_create(self._ctx, int(decimation), _hp(t), int(t.size), 1 if complex_taps else 0,
                                          1 if use_time else 0, C.byref(self._h)), "mi355_filter_create")

    def taps(self):
        n = self._L.mi355_filter_ntaps(self._h)
        out = np.empty(n, np.complex64 if self._complex else np.float32)
        check(min(self._L.mi355_filter_get_taps(self._h, _hp(out), n), 0), "mi355_filter_get_taps")
        return out

    def ntaps(self):
        return self._L.mi355_filter_ntaps(self._h)

    def set_taps2(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.complex64 if self._complex else np.float32)
        check(self._L.mi355_filter_set_taps(self._h, _hp(t), int(t.size)), "mi355_filter_set_taps")

    set_taps = set_taps2

    def history(self):
        return self.ntaps()

    def fftsize(self):
        return self._L.mi355_filter_fftsize(self._h)

    def set_nthreads(self, n):  # lib/clFilter_impl.cc:413-415: only meaningful for the CPU FFTW plan
        pass

    def work(self, noutput_items, input_items, output_items):
        """input_items[0] is the history-prefixed buffer: noutput*decim + ntaps-1 items."""
        x = _host(input_items[0], np.complex64)
        need = noutput_items * self.decimation + self.ntaps() - 1
        if x.size < need:
            raise ValueError("filter work(): need %d input items (history included), got %d" % (need, x.size))
        y = _host(output_items[0], np.complex64, writable=True)
        check(self._L.mi355_filter_work(self._h, noutput_items, _hp(x), _hp(y)), "mi355_filter_work")
        return noutput_items

    def testOpenCL(self, noutput_items, input_items, output_items):
        return self.work(noutput_items, input_items, output_items)

    def work_device(self, noutput_items, input_items, output_items):
        need = int(noutput_items) * self.decimation + self.ntaps() - 1  # history-prefixed input, like work()
        check(self._L.mi355_filter_work_dev(self._h, noutput_items, _dp(input_items[0], need * 8, "input"),
                                            _dp(output_items[0], int(noutput_items) * 8, "output"),
                                            _torch_stream(self.device)), "mi355_filter_work_dev")
        return noutput_items

    def last_route(self):
        """The kernel the last work() / work_device() launched and its parameters (mi355_filter_last_route); "" before the first call."""
        return self._L.mi355_filter_last_route(self._h).decode()


class clFilter(_FilterBase):
    """clFilter::make(openclPlatform, devSelector, platformId, devId, decimation, taps,
    nthreads=1, setDebug=0, use_time=False)  -- include/clenabled/clFilter.h:52-53"""

    def __init__(self, openclPlatform, devSelector, platformId, devId, decimation, taps, nthreads=1, setDebug=0,
                 use_time=False):
        super().__init__(openclPlatform, devSelector, platformId, devId, setDebug)
        self._create(decimation, taps, False, use_time)


class clComplexFilter(_FilterBase):
    """clComplexFilter::make(openclPlatform, devSelector, platformId, devId, decimation,
    taps, nthreads=1, setDebug=0)  -- include/clenabled/clComplexFilter.h:706
    The reference only has the time-domain kernel for complex taps; ``use_time``
    is an additive keyword selecting the fast-convolution kernel instead."""

    def __init__(self, openclPlatform, devSelector, platformId, devId, decimation, taps, nthreads=1, setDebug=0,
                 use_time=True):
        super().__init__(openclPlatform, devSelector, platformId, devId, setDebug)
        self._create(decimation, taps, True, use_time)


class clPolyphaseChannelizer(_Block):
    """clPolyphaseChannelizer::make(openCLPlatformType, devSelector, platformId, devId, taps,
    buf_items, num_channels, ninputs_per_iter, ch_map, setDebug=0)
    -- include/clenabled/clPolyphaseChannelizer.h:48-49"""
    _destroy = "mi355_pfb_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, taps, buf_items, num_channels,
                 ninputs_per_iter, ch_map, setDebug=0):
        if buf_items % num_channels != 0:
            # lib/clPolyphaseChannelizer_impl.cc:59-62
            raise ValueError("buf_items must be a multiple of num_channels")
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        m = np.ascontiguousarray(ch_map, dtype=np.int32)
        self._ntaps = int(t.size)
        self.buf_items = int(buf_items)
        check(self._L.mi355_pfb_create(self._ctx, _hp(t), int(t.size), int(buf_items), int(num_channels),
                                       int(ninputs_per_iter), _hp(m), int(m.size), C.byref(self._h)), "mi355_pfb_create")

    def history(self):
        return self._ntaps

    def noutput(self):
        return self._L.mi355_pfb_noutput(self._h)

    def ninput(self):
        return self._L.mi355_pfb_ninput(self._h)

    def general_work(self, noutput_items, ninput_items, input_items, output_items):
        x = _host(input_items[0], np.complex64)
        if x.size < self.ninput():
            raise ValueError("pfb general_work(): need %d input items (history included)" % self.ninput())
        y = _host(output_items[0], np.complex64, writable=True)
        check(self._L.mi355_pfb_work(self._h, _hp(x), _hp(y)), "mi355_pfb_work")
        return self.noutput()

    def work_device(self, input_items, output_items, nbuf=1):
        """Device-resident call; nbuf > 1: that many consecutive buffers of the stream in one launch (general_work() with
        noutput_items = nbuf * noutput()); input nbuf * buf_items - ninputs_per_iter + ntaps items, output nbuf * noutput()."""
        nbuf = int(nbuf)
        nin = (self.ninput() + (nbuf - 1) * self.buf_items) * 8  # k buffers of the stream share the history in front
        nout = nbuf * self.noutput() * 8
        if nbuf == 1:
            check(self._L.mi355_pfb_work_dev(self._h, _dp(input_items[0], nin, "input"), _dp(output_items[0], nout, "output"),
                                             _torch_stream(self.device)), "mi355_pfb_work_dev")
            return self.noutput()
        x, y = input_items[0], output_items[0]
        check(self._L.mi355_pfb_work_dev_n(self._h, nbuf, _dp(x, nin, "input"), _dp(y, nout, "output"), _torch_stream(self.device)),
              "mi355_pfb_work_dev_n")
        return nbuf * self.noutput()

    def last_route(self):
        """The kernels the last call launched (mi355_pfb_last_route); "" before the first call."""
        return self._L.mi355_pfb_last_route(self._h).decode()


class clXEngine(_Block):
    """clXEngine::make(openCLPlatformType, devSelector, platformId, devId, setDebug, data_type,
    polarization, num_inputs, output_format, first_channel, num_channels, integration,
    antenna_list, ...)  -- include/clenabled/clXEngine.h:48-52.  Only the
    correlation path (xcorrelate / frame gather) is implemented; file/PDU output
    arguments are accepted and ignored."""
    _destroy = "mi355_xengine_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, setDebug, data_type, polarization, num_inputs,
                 output_format, first_channel, num_channels, integration, antenna_list=(), output_file=False,
                 file_base="", rollover_size_mb=0, internal_synchronizer=False, sync_timestamp=0, object_name="",
                 starting_chan_center_freq=0.0, channel_width=0.0, disable_output=False, pipeline_integration=0):
        if num_inputs < 2:
            # lib/clXEngine_impl.cc:106-109
            raise IndexError("Please specify at least 2 inputs to correlate.")
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self.data_type = data_type
        self.npol = 2 if data_type == DTYPE_PACKEDXY else int(polarization)
        self.num_inputs, self.num_channels, self.integration = int(num_inputs), int(num_channels), int(integration)
        self.pipeline_integration = int(pipeline_integration)
        check(self._L.mi355_xengine_create(self._ctx, int(data_type), self.npol, int(num_inputs), int(num_channels),
                                           int(integration), C.byref(self._h)), "mi355_xengine_create")

    def get_input_buffer_size(self):  # lib/clXEngine_impl.h:176 (items, not bytes)
        return self.num_inputs * self.num_channels * self.npol * self.integration

    def input_bytes(self):
        return self._L.mi355_xengine_input_bytes(self._h)

    def get_output_buffer_size(self):
        return self._L.mi355_xengine_output_items(self._h)

    def xcorrelate(self, input_matrix, cross_correlation, accumulate=False):
        """xcorrelate(char*/XComplex* input_matrix, XComplex* cross_correlation)
        -- lib/clXEngine_impl.h:179-201, followed by the blocking read-back of
        runThread (lib/clXEngine_impl.cc:1257)."""
        x = np.ascontiguousarray(input_matrix)
        if x.nbytes < self.input_bytes():
            raise ValueError("xcorrelate: input needs %d bytes" % self.input_bytes())
        y = _host(cross_correlation, np.complex64, writable=True)
        check(self._L.mi355_xengine_xcorrelate(self._h, _hp(x), _hp(y), 1 if accumulate else 0), "mi355_xengine_xcorrelate")
        return self.get_output_buffer_size()

    def submit(self, input_matrix, accumulator=None):
        """Asynchronous xcorrelate: enqueue one integration (at most two in flight); the pinned
        double buffers + worker thread of start()/runThread() (lib/clXEngine_impl.cc:304-382,1234-1299)."""
        x = np.ascontiguousarray(input_matrix)
        if x.nbytes < self.input_bytes():
            raise ValueError("submit: input needs %d bytes" % self.input_bytes())
        acc = None if accumulator is None else _hp(_host(accumulator, np.complex64))
        check(self._L.mi355_xengine_submit(self._h, _hp(x), acc), "mi355_xengine_submit")

    def wait(self, cross_correlation):
        """Block for the oldest submitted integration and return its matrix."""
        y = _host(cross_correlation, np.complex64, writable=True)
        check(self._L.mi355_xengine_wait(self._h, _hp(y)), "mi355_xengine_wait")
        return self.get_output_buffer_size()

    def pending(self):
        return self._L.mi355_xengine_pending(self._h)

    def acquire(self):
        """Zero-copy submit: the pinned frame buffer of the next free slot as a writable int8 numpy view (the
        reference's pinned char_input / complex_input, lib/clXEngine_impl.cc:325-362); fill it, then submit_acquired()."""
        p = C.c_void_p()
        check(self._L.mi355_xengine_acquire(self._h, C.byref(p)), "mi355_xengine_acquire")
        buf = (C.c_int8 * self.input_bytes()).from_address(p.value)
        return np.frombuffer(buf, dtype=np.int8)

    def submit_acquired(self, accumulator=None):
        acc = None if accumulator is None else _hp(_host(accumulator, np.complex64))
        check(self._L.mi355_xengine_submit_acquired(self._h, acc), "mi355_xengine_submit_acquired")

    def xcorrelate_device(self, input_matrix, cross_correlation, accumulate=False, stations_per_group=None):
        """Device-resident xcorrelate.  stations_per_group: the input is the receive buffer of the multi-GPU corner turn,
        [group][t][station in group][chan][pol] (gr-clenabled_amd/shard.py), read in place."""
        nin, nout = self.input_bytes(), self.get_output_buffer_size() * 8
        if stations_per_group:
            check(self._L.mi355_xengine_xcorrelate_grouped_dev(self._h, _dp(input_matrix, nin, "input"), _dp(cross_correlation, nout, "output"), 1 if accumulate else 0,
                                                               int(stations_per_group), _torch_stream(self.device)),
                  "mi355_xengine_xcorrelate_grouped_dev")
            return self.get_output_buffer_size()
        check(self._L.mi355_xengine_xcorrelate_dev(self._h, _dp(input_matrix, nin, "input"), _dp(cross_correlation, nout, "output"),
                                                   1 if accumulate else 0, _torch_stream(self.device)),
              "mi355_xengine_xcorrelate_dev")
        return self.get_output_buffer_size()

    def xcorrelate_n_device(self, nint, input_matrices, cross_correlations, accumulate=False, stations_per_group=None):
        """nint integration windows in one launch (the per-integration loop of lib/clXEngine_impl.cc:1234-1299, batched).  input_matrices:
        nint windows back to back, or with stations_per_group the receive buffer of ONE all-to-all over nint windows,
        [group][window][t][station in group][chan][pol]; cross_correlations: nint matrices back to back."""
        check(self._L.mi355_xengine_xcorrelate_n_dev(self._h, int(nint), _dp(input_matrices, int(nint) * self.input_bytes(), "input"),
                                                     _dp(cross_correlations, int(nint) * self.get_output_buffer_size() * 8, "output"), 1 if accumulate else 0,
                                                     int(stations_per_group or 0), _torch_stream(self.device)),
              "mi355_xengine_xcorrelate_n_dev")
        return nint * self.get_output_buffer_size()

    def pack3d_device(self, dst, src, width_bytes, rows, nblocks, src_pitch, src_block_stride, dst_pitch, dst_block_stride):
        """Strided device copy on this block's context (the send-side packing of the corner turn)."""
        if min(int(width_bytes), int(rows), int(nblocks)) <= 0:
            return  # (nothing to copy: the C call returns at once too)
        # the last byte touched: the last row of the last block
        src_bytes = (int(nblocks) - 1) * int(src_block_stride) + (int(rows) - 1) * int(src_pitch) + int(width_bytes)
        dst_bytes = (int(nblocks) - 1) * int(dst_block_stride) + (int(rows) - 1) * int(dst_pitch) + int(width_bytes)
        check(self._L.mi355_pack3d_dev(self._ctx, _dp(dst, dst_bytes, "destination"), _dp(src, src_bytes, "source"), int(width_bytes), int(rows), int(nblocks), int(src_pitch),
                                       int(src_block_stride), int(dst_pitch), int(dst_block_stride), _torch_stream(self.device)),
              "mi355_pack3d_dev")

    def last_route(self):
        """Which kernels the last device-side call ran (mi355_xengine_last_route): a dict of mi355_xe_route's fields."""
        class Route(C.Structure):
            _fields_ = [("kernel", C.c_char * 64)] + [(k, C.c_int) for k in ("launches", "windows", "workgroups", "units_per_workgroup", "tsplit",
                                                                           "in_launch_reduce", "touches", "pace")]
        r = Route()
        check(self._L.mi355_xengine_last_route(self._h, C.byref(r)), "mi355_xengine_last_route")
        d = {k: int(getattr(r, k)) for k, _ in Route._fields_[1:]}
        d["kernel"] = r.kernel.decode()
        return d

    def selftest_scale(self):
        """Sums S in [-2^24, 2^24] whose single-precision IChar scale differs from (float)((double)S / 127 / 127): must be 0."""
        n = C.c_longlong(-1)
        check(self._L.mi355_xengine_selftest_scale(self._ctx, C.byref(n)), "mi355_xengine_selftest_scale")
        return int(n.value)

    def gather(self, nframes, frame0, input_items, frame_buffer):
        """Host frame gather of work_processor (lib/clXEngine_impl.cc:987-1061)."""
        ins = [np.ascontiguousarray(x) for x in input_items]
        p = (C.c_void_p * len(ins))(*[x.ctypes.data for x in ins])
        check(self._L.mi355_xengine_gather(self._h, int(nframes), int(frame0), p, _hp(frame_buffer)), "mi355_xengine_gather")
        return nframes


class clXEngineSharded:
    """clXEngine over several devices of one process: `world` ranks on devices `device_ids` (mi355_xengine_shard_*, the single-process
    counterpart of shard.py).  IChar only.  The reference has no such class -- it picks ONE device per block (devId,
    lib/GRCLBase.cpp:115-134); this is the form a flowgraph (one process) can use.  xcorrelate(): `windows` integration windows in the
    reference's frame layout in, `windows` triangular-order matrices out (lib/clXEngine_impl.h:179-201 over the devices)."""

    def __init__(self, device_ids, polarization, num_inputs, num_channels, integration, windows=1):
        self._L = lib()
        self._h = C.c_void_p()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        self.world, self.npol, self.windows = len(device_ids), int(polarization), int(windows)
        self.num_inputs, self.num_channels, self.integration = int(num_inputs), int(num_channels), int(integration)
        check(self._L.mi355_xengine_shard_create(self.world, ids, self.npol, self.num_inputs, self.num_channels, self.integration, self.windows,
                                                 C.byref(self._h)), "mi355_xengine_shard_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.mi355_xengine_shard_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frames_bytes(self):
        return self._L.mi355_xengine_shard_frames_bytes(self._h)

    def slab_items(self):
        return self._L.mi355_xengine_shard_slab_items(self._h)

    def get_output_buffer_size(self):  # items of ONE window's full matrix
        return self.slab_items() * self.world

    def device(self, rank):
        return self._L.mi355_xengine_shard_device(self._h, int(rank))

    def stream(self, rank):
        return self._L.mi355_xengine_shard_stream(self._h, int(rank))

    def xcorrelate(self, input_matrix, cross_correlation, accumulate=False):
        x = np.ascontiguousarray(input_matrix)
        need = self.windows * self.integration * self.num_inputs * self.num_channels * self.npol * 2
        if x.nbytes < need:
            raise ValueError("xcorrelate: input needs %d bytes" % need)
        y = _host(cross_correlation, np.complex64, writable=True)
        if y.size < self.windows * self.get_output_buffer_size():
            raise ValueError("xcorrelate: output needs %d items" % (self.windows * self.get_output_buffer_size()))
        check(self._L.mi355_xengine_shard_xcorrelate(self._h, _hp(x), _hp(y), 1 if accumulate else 0), "mi355_xengine_shard_xcorrelate")
        return self.windows * self.get_output_buffer_size()

    def input_bytes(self):
        return self._L.mi355_xengine_shard_input_bytes(self._h)

    def acquire(self):
        """Streaming host path: the pinned frame buffer of the next free slot (`windows` integration windows in the reference's frame layout,
        lib/clXEngine_impl.cc:325-362) as a writable int8 numpy view; fill it, then submit_acquired()."""
        p = C.c_void_p()
        check(self._L.mi355_xengine_shard_acquire(self._h, C.byref(p)), "mi355_xengine_shard_acquire")
        return np.frombuffer((C.c_int8 * self.input_bytes()).from_address(p.value), dtype=np.int8)

    def submit_acquired(self):
        """Per rank, on its own stream: upload of its antenna group out of the pinned buffer, exchange, correlation, download -- enqueue only."""
        check(self._L.mi355_xengine_shard_submit_acquired(self._h), "mi355_xengine_shard_submit_acquired")

    def wait(self, cross_correlation):
        """Block for the oldest submitted exchange; `windows` matrices."""
        y = _host(cross_correlation, np.complex64, writable=True)
        if y.size < self.windows * self.get_output_buffer_size():
            raise ValueError("wait: output needs %d items" % (self.windows * self.get_output_buffer_size()))
        check(self._L.mi355_xengine_shard_wait(self._h, _hp(y)), "mi355_xengine_shard_wait")
        return self.windows * self.get_output_buffer_size()

    def pending(self):
        return self._L.mi355_xengine_shard_pending(self._h)

    def submit_device(self, frames, outs, accumulate=False):
        """frames[r] / outs[r]: CUDA tensors on the rank's device (antenna-group frames / windows x slab matrices); enqueue only."""
        fp = (C.c_void_p * self.world)(*[_dp(t, self.frames_bytes(), "frames").value for t in frames])
        op = (C.c_void_p * self.world)(*[_dp(t, self.windows * self.slab_items() * 8, "output").value for t in outs])
        check(self._L.mi355_xengine_shard_submit_dev(self._h, fp, op, 1 if accumulate else 0), "mi355_xengine_shard_submit_dev")

    def wait_current_stream(self, rank):
        """The rank's compute stream waits for everything enqueued so far on torch's current stream of the rank's device."""
        check(self._L.mi355_xengine_shard_wait_stream(self._h, int(rank), _torch_stream(self.device(rank))), "mi355_xengine_shard_wait_stream")

    def synchronize(self):
        check(self._L.mi355_xengine_shard_synchronize(self._h), "mi355_xengine_shard_synchronize")


class _Elem(_Block):
    """Remaining elementwise family over mi355_elem_*."""
    _destroy = "mi355_elem_destroy"
    _kind = 0
    _in = ()
    _out = ()

    def _create(self, p0=0.0, p1=0.0):
        check(self._L.mi355_elem_create(self._ctx, self._kind, float(p0), float(p1), C.byref(self._h)), "mi355_elem_create")

    def history(self):
        return self._L.mi355_elem_history(self._h)

    def work(self, noutput_items, input_items, output_items):
        ins = [_host(x, t) for x, t in zip(input_items, self._in)]
        need = noutput_items + self.history() - 1
        if any(x.size < need for x in ins):
            raise ValueError("work(): need %d input items (history included)" % need)
        outs = [_host(y, t, writable=True) for y, t in zip(output_items, self._out)]
        check(self._L.mi355_elem_work(self._h, noutput_items, _hp(ins[0]), _hp(ins[1]) if len(ins) > 1 else None,
                                      _hp(outs[0]), _hp(outs[1]) if len(outs) > 1 else None), "mi355_elem_work")
        return noutput_items

    testOpenCL = work

    def work_device(self, noutput_items, input_items, output_items):
        i, o = input_items, output_items
        nin = [(int(noutput_items) + self.history() - 1) * np.dtype(t).itemsize for t in self._in]
        nout = [int(noutput_items) * np.dtype(t).itemsize for t in self._out]
        check(self._L.mi355_elem_work_dev(self._h, noutput_items, _dp(i[0], nin[0], "input 0"), _dp(i[1], nin[1], "input 1") if len(self._in) > 1 else None,
                                          _dp(o[0], nout[0], "output 0"), _dp(o[1], nout[1], "output 1") if len(self._out) > 1 else None,
                                          _torch_stream(self.device)), "mi355_elem_work_dev")
        return noutput_items


class clLog(_Elem):
    """clLog::make(openCLPlatformType, devSelector, platformId, devId, nValue, kValue, setDebug=0) -- clLog.h:49"""
    _kind, _in, _out = 1, (np.float32,), (np.float32,)

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, nValue, kValue, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self._create(nValue, kValue)


class clSNR(_Elem):
    """clSNR::make(openCLPlatformType, devSelector, platformId, devId, nValue, kValue, setDebug=0) -- clSNR.h:49"""
    _kind, _in, _out = 2, (np.float32, np.float32), (np.float32,)

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, nValue, kValue, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self._create(nValue, kValue)


class clComplexToMag(_Elem):
    """clComplexToMag::make(openCLPlatformType, devSelector, platformId, devId, setDebug=0) -- clComplexToMag.h:49"""
    _kind, _in, _out = 3, (np.complex64,), (np.float32,)

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self._create()


class clComplexToArg(clComplexToMag):
    """clComplexToArg::make(...) -- clComplexToArg.h:49"""
    _kind = 4


class clComplexToMagPhase(clComplexToMag):
    """clComplexToMagPhase::make(...) -- clComplexToMagPhase.h:49; outputs (mag, phase)"""
    _kind, _out = 5, (np.float32, np.float32)


class clMagPhaseToComplex(clComplexToMag):
    """clMagPhaseToComplex::make(...) -- clMagPhaseToComplex.h:49; inputs (mag, phase)"""
    _kind, _in, _out = 6, (np.float32, np.float32), (np.complex64,)


class clQuadratureDemod(_Elem):
    """clQuadratureDemod::make(gain, openCLPlatformType, devSelector, platformId, devId, setDebug=0)
    -- clQuadratureDemod.h:49; history 2 (lib/clQuadratureDemod_impl.cc:81)"""
    _kind, _in, _out = 7, (np.complex64,), (np.float32,)

    def __init__(self, gain, openCLPlatformType, devSelector, platformId, devId, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self._create(gain, 0.0)


class clxcorrelate_fft_vcf(_Block):
    """clxcorrelate_fft_vcf::make(fftSize, num_inputs, openCLPlatformType, devSelector, platformId, devId, input_type=1)
    -- include/clenabled/clxcorrelate_fft_vcf.h:50.  Input 0 is the reference; output s-1 is the half-swapped magnitude of
    the unscaled inverse FFT of X0 * conj(Xs) (lib/clxcorrelate_fft_vcf_impl.cc:1058-1143).  input_type 1 = the inputs
    are spectra, 2 = time series (forward FFT first)."""
    _destroy = "mi355_xcorr_fft_destroy"

    def __init__(self, fftSize, num_inputs, openCLPlatformType, devSelector, platformId, devId, input_type=1):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, 0)
        self.fft_size, self.num_inputs, self.input_type = int(fftSize), int(num_inputs), int(input_type)
        check(self._L.mi355_xcorr_fft_create(self._ctx, self.fft_size, self.num_inputs, self.input_type, C.byref(self._h)),
              "mi355_xcorr_fft_create")

    def work(self, noutput_items, input_items, output_items):
        if len(input_items) != self.num_inputs or len(output_items) != self.num_inputs - 1:
            raise ValueError("work(): %d inputs and %d outputs expected" % (self.num_inputs, self.num_inputs - 1))
        ins = [_host(x, np.complex64) for x in input_items]
        outs = [_host(y, np.float32, writable=True) for y in output_items]
        need = noutput_items * self.fft_size
        if any(x.size < need for x in ins) or any(y.size < need for y in outs):
            raise ValueError("work(): every buffer must hold noutput_items vectors of fft_size items")
        ip = (C.c_void_p * len(ins))(*[_hp(x) for x in ins])
        op = (C.c_void_p * len(outs))(*[_hp(y) for y in outs])
        check(self._L.mi355_xcorr_fft_work(self._h, noutput_items, ip, op), "mi355_xcorr_fft_work")
        return noutput_items

    work_test = work

    def work_device(self, noutput_items, input_items, output_items):
        if len(input_items) != self.num_inputs or len(output_items) != self.num_inputs - 1:
            raise ValueError("work_device(): %d inputs and %d outputs expected" % (self.num_inputs, self.num_inputs - 1))
        need = int(noutput_items) * self.fft_size
        ip = (C.c_void_p * len(input_items))(*[_dp(x, need * 8, "input %d" % k).value for k, x in enumerate(input_items)])
        op = (C.c_void_p * len(output_items))(*[_dp(y, need * 4, "output %d" % k).value for k, y in enumerate(output_items)])
        check(self._L.mi355_xcorr_fft_work_dev(self._h, noutput_items, ip, op, _torch_stream(self.device)), "mi355_xcorr_fft_work_dev")
        return noutput_items


class clXCorrelate(_Block):
    """clXCorrelate::make(openCLPlatformType, devSelector, platformId, devId, setDebug, num_inputs, signal_length, data_type,
    data_size, max_search_index, decim_frames, async=false) -- include/clenabled/clXCorrelate.h:55-56 (``async`` is a Python
    keyword: the keyword form here is ``async_``).  Time-domain lag search of inputs 1..num_inputs-1 against input 0; every
    processed frame publishes a PDU ``{"corrvect": float32[num_inputs-1], "corrective_lags": int32[num_inputs-1]}`` on port
    "corr" (lib/clXCorrelate_impl.cc:1594-1600), read here with pop_pdu().  decim_frames and async follow work() (:1529-1645):
    with async the frame is submitted and work() returns at once; the result of the previous submission is published when the
    next frame is accepted, and frames arriving while a submission runs pass through uncounted."""
    _destroy = "mi355_xcorr_td_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, setDebug, num_inputs, signal_length, data_type,
                 data_size, max_search_index, decim_frames, async_=False):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self.num_inputs, self.signal_length = int(num_inputs), int(signal_length)
        self.data_type, self.decim_frames, self.async_ = int(data_type), int(decim_frames), bool(async_)
        check(self._L.mi355_xcorr_td_create(self._ctx, self.num_inputs, self.signal_length, self.data_type, int(data_size),
                                            int(max_search_index), C.byref(self._h)), "mi355_xcorr_td_create")
        self.max_shift = self._L.mi355_xcorr_td_max_shift(self._h)
        self._np = np.complex64 if self.data_type == DTYPE_COMPLEX else np.float32
        self._counter = 1           # cur_frame_counter (:708)
        self._pending = False       # a submission not yet collected
        self._ready = None          # its result, once collected, waiting for the next accepted frame
        self._pdus = []

    def message_ports_out(self):
        return ["corr"]

    def pop_pdu(self):
        """The oldest published PDU as a dict, or None."""
        return self._pdus.pop(0) if self._pdus else None

    def _inputs(self, input_items):
        if len(input_items) != self.num_inputs:
            raise ValueError("work(): %d inputs expected" % self.num_inputs)
        ins = [_host(np.asarray(x).reshape(-1)[:self.signal_length], self._np) for x in input_items]
        for k, x in enumerate(ins):
            _need("input %d" % k, x, self.signal_length)
        return ins, (C.c_void_p * len(ins))(*[_hp(x) for x in ins])

    def _result(self):
        n = self.num_inputs - 1
        return np.empty(n, np.float32), np.empty(n, np.int32)

    def _publish(self, corr, lags):
        self._pdus.append({"corrvect": corr, "corrective_lags": lags})

    def _decimate(self):
        """True if this frame is processed (:1539-1546 / :1607-1615)."""
        if self.decim_frames > 1:
            c = self._counter
            self._counter += 1
            if c % self.decim_frames != 0:
                return False
            self._counter = 1
        return True

    def work(self, noutput_items, input_items, output_items=None):
        """One frame of signal_length items per input; returns signal_length (0 if fewer items are available)."""
        n = self.signal_length
        if noutput_items < n:
            return 0
        if not self.async_:
            if not self._decimate():
                return n
            ins, ip = self._inputs(input_items)
            corr, lags = self._result()
            check(self._L.mi355_xcorr_td_work(self._h, ip, _hp(corr), _hp(lags)), "mi355_xcorr_td_work")
            self._publish(corr, lags)
            return n
        if self._pending:
            corr, lags = self._result()
            r = self._L.mi355_xcorr_td_poll(self._h, _hp(corr), _hp(lags))
            if r < 0:
                check(r, "mi355_xcorr_td_poll")
            if r == 0:
                return n  # still running: the frame passes through, uncounted
            self._pending, self._ready = False, (corr, lags)
        if not self._decimate():
            return n
        ins, ip = self._inputs(input_items)
        if self._ready is not None:
            self._publish(*self._ready)
            self._ready = None
        check(self._L.mi355_xcorr_td_submit(self._h, ip), "mi355_xcorr_td_submit")
        self._pending = True
        return n

    def wait(self):
        """Block until the running submission (if any) has finished (test / shutdown aid; its result is published with the next
        accepted frame)."""
        check(self._L.mi355_xcorr_td_wait(self._h), "mi355_xcorr_td_wait")

    def work_device(self, nframes, input_items, corr, lags, curves=None):
        """Device path: input_items = num_inputs CUDA tensors of [nframes][signal_length] items; corr (float32) and lags (int32)
        of [nframes][num_inputs-1]; curves (float32, [nframes][num_inputs-1][2*max_shift]) or None.  Enqueued on torch's
        current stream."""
        nf, nsig = int(nframes), self.num_inputs - 1
        isz = 8 if self.data_type == DTYPE_COMPLEX else 4
        if len(input_items) != self.num_inputs:
            raise ValueError("work_device(): %d inputs expected" % self.num_inputs)
        ip = (C.c_void_p * self.num_inputs)(*[_dp(x, nf * self.signal_length * isz, "input") for x in input_items])
        cv = _dp(curves, nf * nsig * 2 * self.max_shift * 4, "curves") if curves is not None else C.c_void_p()
        check(self._L.mi355_xcorr_td_work_dev(self._h, nf, ip, _dp(corr, nf * nsig * 4, "corr"), _dp(lags, nf * nsig * 4, "lags"), cv,
                                              _torch_stream(self.device)), "mi355_xcorr_td_work_dev")
        return nf


class clSignalSource(_Block):
    """clSignalSource::make(idataType, openCLPlatformType, devSelector, platformId, devId, samp_rate, waveform, freq, amplitude,
    setDebug=0) -- include/clenabled/clSignalSource.h:49-50.  NCO / tone generator: waveform 1 cos, 2 sin (complex output carries
    both); the phase advances from call to call and is kept by set_frequency()."""
    _destroy = "mi355_sigsource_destroy"

    def __init__(self, idataType, openCLPlatformType, devSelector, platformId, devId, samp_rate, waveform, freq, amplitude, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self.dtype = int(idataType)
        check(self._L.mi355_sigsource_create(self._ctx, self.dtype, float(samp_rate), int(waveform), float(freq), float(amplitude),
                                             C.byref(self._h)), "mi355_sigsource_create")

    def set_frequency(self, freq):
        check(self._L.mi355_sigsource_set_frequency(self._h, float(freq)), "mi355_sigsource_set_frequency")

    def set_phase(self, angle_pos):
        check(self._L.mi355_sigsource_set_phase(self._h, float(angle_pos)), "mi355_sigsource_set_phase")

    def get_state(self):
        """(angle_pos, angle_rate_inc): the phase of the next call's first item and the phase step per item, in radians"""
        pos, inc = C.c_double(), C.c_double()
        check(self._L.mi355_sigsource_get_state(self._h, C.byref(pos), C.byref(inc)), "mi355_sigsource_get_state")
        return pos.value, inc.value

    def work(self, noutput_items, input_items, output_items):
        c = _host(output_items[0], _NP_OF[self.dtype], writable=True)
        _need("output", c, noutput_items)
        check(self._L.mi355_sigsource_work(self._h, noutput_items, _hp(c)), "mi355_sigsource_work")
        return noutput_items

    testOpenCL = work

    def work_device(self, noutput_items, input_items, output_items):
        nb = int(noutput_items) * np.dtype(_NP_OF[self.dtype]).itemsize
        check(self._L.mi355_sigsource_work_dev(self._h, noutput_items, _dp(output_items[0], nb, "output"), _torch_stream(self.device)),
              "mi355_sigsource_work_dev")
        return noutput_items


class clCostasLoop(_Block):
    """clCostasLoop::make(openCLPlatformType, devSelector, platformId, devId, loop_bw, order, setDebug=0) --
    include/clenabled/clCostasLoop.h:52; order 2 (BPSK) or 4 (QPSK).  num_streams (not in the reference) runs one loop per stream
    of an item-major multiplex, item i of stream s at [i * num_streams + s] -- the channelizer's output layout.  Output 0 is the
    de-rotated stream; the optional output 1 is the loop frequency (float, rad/item) per item.  The loop state lives on the
    device, so work_device() calls chain."""
    _destroy = "mi355_costas_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, loop_bw, order, setDebug=0, num_streams=1):
        L = lib()
        a, b = C.c_float(), C.c_float()
        rc = L.mi355_costas_plan(float(loop_bw), int(order), C.byref(a), C.byref(b))
        if rc == -1:
            raise ValueError(L.mi355_last_error().decode())  # std::invalid_argument, lib/clCostasLoop_impl.cc:80-83
        check(rc, "mi355_costas_plan")
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self.order, self.num_streams, self._bw = int(order), int(num_streams), float(loop_bw)
        self._alpha, self._beta = a.value, b.value
        check(self._L.mi355_costas_create(self._ctx, self._bw, self.order, self.num_streams, C.byref(self._h)), "mi355_costas_create")

    def set_loop_bandwidth(self, loop_bw):
        a, b = C.c_float(), C.c_float()
        check(self._L.mi355_costas_set_loop_bandwidth(self._h, float(loop_bw)), "mi355_costas_set_loop_bandwidth")
        check(self._L.mi355_costas_plan(float(loop_bw), self.order, C.byref(a), C.byref(b)), "mi355_costas_plan")
        self._bw, self._alpha, self._beta = float(loop_bw), a.value, b.value

    def get_loop_bandwidth(self):
        return self._bw

    def get_alpha(self):
        return self._alpha

    def get_beta(self):
        return self._beta

    def get_state(self):
        """(phase, freq, error): float64 arrays of num_streams values; waits for the block's last call"""
        st = [np.empty(self.num_streams, np.float64) for _ in range(3)]
        check(self._L.mi355_costas_get_state(self._h, _hp(st[0]), _hp(st[1]), _hp(st[2])), "mi355_costas_get_state")
        return tuple(st)

    def set_state(self, phase=None, freq=None):
        """phase / freq: a scalar (every stream) or num_streams values; None leaves that part as it is"""
        arrs = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (self.num_streams,)))
                for v in (phase, freq)]
        check(self._L.mi355_costas_set_state(self._h, *[C.c_void_p() if a is None else _hp(a) for a in arrs]), "mi355_costas_set_state")

    def get_phase(self):
        p = self.get_state()[0]
        return float(p[0]) if self.num_streams == 1 else p

    def get_frequency(self):
        f = self.get_state()[1]
        return float(f[0]) if self.num_streams == 1 else f

    def set_phase(self, phase):
        self.set_state(phase=phase)

    def set_frequency(self, freq):
        self.set_state(freq=freq)

    def work(self, noutput_items, input_items, output_items):
        n = int(noutput_items) * self.num_streams
        a = _host(input_items[0], np.complex64)
        c = _host(output_items[0], np.complex64, writable=True)
        _need("input", a, n)
        _need("output", c, n)
        fo = None
        if len(output_items) > 1 and output_items[1] is not None:
            fo = _host(output_items[1], np.float32, writable=True)
            _need("frequency output", fo, n)
        check(self._L.mi355_costas_work(self._h, noutput_items, _hp(a), _hp(c), _hp(fo) if fo is not None else C.c_void_p()),
              "mi355_costas_work")
        return noutput_items

    testOpenCL = work

    def work_device(self, noutput_items, input_items, output_items):
        n = int(noutput_items) * self.num_streams
        fo = C.c_void_p()
        if len(output_items) > 1 and output_items[1] is not None:
            fo = _dp(output_items[1], n * 4, "frequency output")
        check(self._L.mi355_costas_work_dev(self._h, noutput_items, _dp(input_items[0], n * 8, "input"),
                                            _dp(output_items[0], n * 8, "output"), fo, _torch_stream(self.device)),
              "mi355_costas_work_dev")
        return noutput_items


class clRationalResampler(_Block):
    """Polyphase FIR with interpolation L and decimation M, the contract of GNU Radio's rational_resampler_ccf / ccc (beyond the
    reference module): y = (taps * zero-stuff_L(x))[phase + m M].  L and M are used as given (not reduced by their gcd) and the
    taps carry the gain L.  Complex taps are detected from the array's dtype.  history() = ceil(ntaps / L) taps per arm; the
    input of a call is history-prefixed like clFilter's, a call returns (noutput, consumed) and the next call's input starts
    `consumed` items later."""
    _destroy = "mi355_resampler_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, interpolation, decimation, taps, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self._interp, self._decim = int(interpolation), int(decimation)
        t = self._taps_array(taps, None)
        check(self._L.mi355_resampler_create(self._ctx, self._interp, self._decim, _hp(t), int(t.size), 1 if self._complex else 0,
                                             C.byref(self._h)), "mi355_resampler_create")

    def _taps_array(self, taps, complex_taps):
        a = np.asarray(taps)
        if complex_taps is None:
            complex_taps = np.iscomplexobj(a)
            self._complex = bool(complex_taps)
        elif np.iscomplexobj(a) and not complex_taps:
            raise TypeError("complex taps for a resampler created with real taps")
        return np.ascontiguousarray(a, dtype=np.complex64 if complex_taps else np.float32).reshape(-1)

    def taps(self):
        n = self.ntaps()
        out = np.empty(n, np.complex64 if self._complex else np.float32)
        check(min(self._L.mi355_resampler_get_taps(self._h, _hp(out), n), 0), "mi355_resampler_get_taps")
        return out

    def ntaps(self):
        return self._L.mi355_resampler_ntaps(self._h)

    def set_taps(self, taps):
        t = self._taps_array(taps, self._complex)
        check(self._L.mi355_resampler_set_taps(self._h, _hp(t), int(t.size)), "mi355_resampler_set_taps")

    def history(self):
        return self._L.mi355_resampler_history(self._h)

    def interpolation(self):
        return self._interp

    def decimation(self):
        return self._decim

    def phase(self):
        c = C.c_int()
        check(self._L.mi355_resampler_get_phase(self._h, C.byref(c)), "mi355_resampler_get_phase")
        return c.value

    def set_phase(self, phase):
        check(self._L.mi355_resampler_set_phase(self._h, int(phase)), "mi355_resampler_set_phase")

    def plan(self, noutput):
        """(consumed, needed, phase_after) of a call of `noutput` items from the current phase; needed counts the history"""
        nt, c = C.c_int(), C.c_int()
        used, need = C.c_longlong(), C.c_longlong()
        check(self._L.mi355_resampler_plan(self._interp, self._decim, self.ntaps(), self.phase(), int(noutput), C.byref(nt), C.byref(used),
                                         C.byref(need), C.byref(c)), "mi355_resampler_plan")
        return used.value, need.value, c.value

    def noutput_for(self, navail):
        """the most outputs a history-prefixed input of `navail` items allows from the current phase"""
        n = self._L.mi355_resampler_noutput_for(self._interp, self._decim, self.ntaps(), self.phase(), int(navail))
        if n < 0:
            check(int(n), "mi355_resampler_noutput_for")
        return int(n)

    def work(self, noutput_items, input_items, output_items):
        """input_items[0] is the history-prefixed buffer; returns (noutput_items, consumed)"""
        x = _host(input_items[0], np.complex64)
        need = self.plan(noutput_items)[1]
        if x.size < need:
            raise ValueError("resampler work(): need %d input items (history included), got %d" % (need, x.size))
        y = _host(output_items[0], np.complex64, writable=True)
        _need("output", y, noutput_items)
        used = C.c_longlong()
        check(self._L.mi355_resampler_work(self._h, int(noutput_items), _hp(x), _hp(y), C.byref(used)), "mi355_resampler_work")
        return noutput_items, used.value

    def work_device(self, noutput_items, input_items, output_items):
        need = self.plan(noutput_items)[1]
        t = input_items[0]
        if t.is_cuda and t.numel() * t.element_size() < need * 8:
            raise ValueError("resampler work_device(): need %d input items (history included), got %d"
                             % (need, t.numel() * t.element_size() // 8))
        used = C.c_longlong()
        check(self._L.mi355_resampler_work_dev(self._h, int(noutput_items), _dp(t, need * 8, "input"),
                                             _dp(output_items[0], int(noutput_items) * 8, "output"), C.byref(used),
                                             _torch_stream(self.device)), "mi355_resampler_work_dev")
        return noutput_items, used.value


class clInterpFIRFilter(clRationalResampler):
    """interp_fir_filter_ccf / ccc: clRationalResampler with decimation 1 -- `interpolation` outputs per input item."""

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, interpolation, taps, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, interpolation, 1, taps, setDebug)


class clPolyphaseSynthesizer(_Block):
    """Critically sampled inverse-DFT polyphase synthesis bank, the counterpart of clPolyphaseChannelizer (beyond the reference
    module; the contract is in include/mi355_clenabled.h).  The input is the channelizer's item-major multiplex -- frames of nmap
    items, slot q feeding channel ch_map[q] (None: all num_channels channels in order) -- history-prefixed with
    history() = (taps_per_arm() - 1) * nmap items; a call for nframes frames writes nframes * num_channels items and the next
    call's input starts nframes * nmap items later.  The taps carry the gain."""
    _destroy = "mi355_synth_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, taps, num_channels, ch_map=None, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self._M = int(num_channels)
        if ch_map is None:
            m, mp, self._nmap = None, C.c_void_p(), self._M
        else:
            m = np.ascontiguousarray(ch_map, dtype=np.int32).reshape(-1)
            mp, self._nmap = _hp(m), int(m.size)
        check(self._L.mi355_synth_create(self._ctx, _hp(t), int(t.size), self._M, mp, self._nmap, C.byref(self._h)), "mi355_synth_create")

    def taps(self):
        n = self.ntaps()
        out = np.empty(n, np.float32)
        check(min(self._L.mi355_synth_get_taps(self._h, _hp(out), n), 0), "mi355_synth_get_taps")
        return out

    def ntaps(self):
        return self._L.mi355_synth_ntaps(self._h)

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        check(self._L.mi355_synth_set_taps(self._h, _hp(t), int(t.size)), "mi355_synth_set_taps")

    def taps_per_arm(self):
        return self._L.mi355_synth_taps_per_arm(self._h)

    def num_channels(self):
        return self._M

    def nmap(self):
        return self._nmap

    def history(self):
        return (self.taps_per_arm() - 1) * self._nmap

    def route(self):
        return self._L.mi355_synth_route(self._h).decode()

    def plan(self, nframes):
        """(ninput_items, noutput_items) of a call of `nframes` frames; ninput_items counts the history"""
        nt = C.c_int()
        nin, nout = C.c_longlong(), C.c_longlong()
        check(self._L.mi355_synth_plan(self.ntaps(), self._M, self._nmap, int(nframes), C.byref(nt), C.byref(nin), C.byref(nout)),
              "mi355_synth_plan")
        return nin.value, nout.value

    def general_work(self, noutput_items, ninput_items, input_items, output_items):
        """host buffers; noutput_items is rounded down to whole frames of num_channels items; returns (produced, consumed)"""
        nframes = int(noutput_items) // self._M
        if nframes == 0:
            return 0, 0
        nin, nout = self.plan(nframes)
        x = _host(input_items[0], np.complex64)
        if x.size < nin:
            raise ValueError("synthesizer general_work(): need %d input items (history included), got %d" % (nin, x.size))
        y = _host(output_items[0], np.complex64, writable=True)
        _need("output", y, nout)
        check(self._L.mi355_synth_work(self._h, nframes, _hp(x), _hp(y)), "mi355_synth_work")
        return nout, nframes * self._nmap

    def work_device(self, nframes, input_items, output_items):
        if int(nframes) == 0:
            return 0
        nin, nout = self.plan(nframes)
        check(self._L.mi355_synth_work_dev(self._h, int(nframes), _dp(input_items[0], nin * 8, "input"),
                                           _dp(output_items[0], nout * 8, "output"), _torch_stream(self.device)), "mi355_synth_work_dev")
        return nout


class clPowerSpectrum(_Block):
    """Averaged power spectrum: window, forward DFT, |X|^2, mean over navg frames, optionally 10 log10 (beyond the reference module;
    the contract is in include/mi355_clenabled.h).  Frames start `hop` items apart (None: fft_size; smaller: Welch overlap; larger:
    the items in between are skipped and never read).  A call for S spectra reads (S * navg - 1) * hop + fft_size complex items,
    history() = max(fft_size - hop, 0) of them shared with the call before, and writes S * fft_size floats; the next call's input
    starts S * navg * hop items later (with hop > fft_size that is past the last item read: general_work(), which reports what it
    consumed, asks for all S * navg * hop items)."""
    _destroy = "mi355_pspec_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, fft_size, navg, window=None, hop=None, shift=False,
                 log_output=False, scale=1.0, setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self._N, self._K = int(fft_size), int(navg)
        self._H = self._N if hop is None else int(hop)
        w, wp, wn = self._window_arg(window)
        check(self._L.mi355_pspec_create(self._ctx, self._N, wp, wn, self._K, self._H, 1 if shift else 0, 1 if log_output else 0,
                                         float(scale), C.byref(self._h)), "mi355_pspec_create")

    @staticmethod
    def _window_arg(window):
        if window is None or len(window) == 0:
            return None, C.c_void_p(), 0
        w = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
        return w, _hp(w), int(w.size)

    def fft_size(self):
        return self._N

    def navg(self):
        return self._K

    def hop(self):
        return self._H

    def history(self):
        return max(self._N - self._H, 0)

    def route(self):
        return self._L.mi355_pspec_route(self._h).decode()

    def set_scale(self, scale):
        check(self._L.mi355_pspec_set_scale(self._h, float(scale)), "mi355_pspec_set_scale")

    def set_window(self, window):
        w, wp, wn = self._window_arg(window)
        check(self._L.mi355_pspec_set_window(self._h, wp, wn), "mi355_pspec_set_window")

    def set_generic(self, on):
        check(self._L.mi355_pspec_set_generic(self._h, 1 if on else 0), "mi355_pspec_set_generic")

    def plan(self, nspectra):
        """(ninput_items, noutput_items) of a call of `nspectra` spectra"""
        nin, nout = C.c_longlong(), C.c_longlong()
        check(self._L.mi355_pspec_plan(self._N, self._K, self._H, int(nspectra), C.byref(nin), C.byref(nout)), "mi355_pspec_plan")
        return nin.value, nout.value

    def work(self, x):
        """host buffer; as many whole spectra as x holds; returns them as a float32 array of shape (nspectra, fft_size)"""
        x = _host(x, np.complex64)
        ns = 0 if x.size < self._N else ((x.size - self._N) // self._H + 1) // self._K
        y = np.empty((ns, self._N), np.float32)
        check(self._L.mi355_pspec_work(self._h, ns, _hp(x), _hp(y)), "mi355_pspec_work")
        return y

    def general_work(self, noutput_items, ninput_items, input_items, output_items):
        """host buffers; noutput_items counts spectra (vectors of fft_size floats); returns (produced, consumed).  The input must hold
        what is consumed, navg * hop per spectrum: with hop > fft_size that is more than the (S * navg - 1) * hop + fft_size items read"""
        ns = int(noutput_items)
        if ns == 0:
            return 0, 0
        nin, nout = self.plan(ns)
        nin = max(nin, ns * self._K * self._H)
        x = _host(input_items[0], np.complex64)
        if x.size < nin:
            raise ValueError("clPowerSpectrum general_work(): need %d input items, got %d" % (nin, x.size))
        y = _host(output_items[0], np.float32, writable=True)
        _need("output", y, nout)
        check(self._L.mi355_pspec_work(self._h, ns, _hp(x), _hp(y)), "mi355_pspec_work")
        return ns, ns * self._K * self._H

    def work_device(self, nspectra, input_items, output_items):
        if int(nspectra) == 0:
            return 0
        nin, nout = self.plan(nspectra)
        check(self._L.mi355_pspec_work_dev(self._h, int(nspectra), _dp(input_items[0], nin * 8, "input"),
                                           _dp(output_items[0], nout * 4, "output"), _torch_stream(self.device)), "mi355_pspec_work_dev")
        return nout


class clFreqXlatingFIRFilter(_Block):
    """Frequency-translating FIR filter, the contract of GNU Radio's freq_xlating_fir_filter_ccf / ccc (beyond the reference module;
    the contract is in include/mi355_clenabled.h): the band at `center_freq` is moved to baseband, filtered with `taps` and decimated.
    `center_freq` is a scalar (one output stream) or a sequence (one output stream per frequency, all formed from one read of the
    input).  Complex taps are detected from the array's dtype.  The input of a call is history-prefixed like clFilter's:
    noutput * decimation + ntaps - 1 items, history() = ntaps.  The phase of every channel is a 64-bit integer kept across calls, so any
    split of a stream into calls gives the same bits."""
    _destroy = "mi355_xlate_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, decimation, taps, center_freq, sampling_freq, use_time=False,
                 setDebug=0):
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        self._decim = int(decimation)
        f = np.ascontiguousarray(np.atleast_1d(np.asarray(center_freq, dtype=np.float64))).reshape(-1)
        self._nch = int(f.size)
        a = np.asarray(taps)
        self._complex = bool(np.iscomplexobj(a))
        t = np.ascontiguousarray(a, dtype=np.complex64 if self._complex else np.float32).reshape(-1)
        check(self._L.mi355_xlate_create(self._ctx, self._decim, _hp(t), int(t.size), 1 if self._complex else 0, float(sampling_freq),
                                         f.ctypes.data_as(C.POINTER(C.c_double)), self._nch, 1 if use_time else 0, C.byref(self._h)),
              "mi355_xlate_create")

    def decimation(self):
        return self._decim

    def num_channels(self):
        return self._nch

    def ntaps(self):
        return self._L.mi355_xlate_ntaps(self._h)

    def history(self):
        return self.ntaps()

    def taps(self):
        n = self.ntaps()
        out = np.empty(n, np.complex64 if self._complex else np.float32)
        check(min(self._L.mi355_xlate_get_taps(self._h, _hp(out), n), 0), "mi355_xlate_get_taps")
        return out

    def set_taps(self, taps):
        a = np.asarray(taps)
        if np.iscomplexobj(a) and not self._complex:
            raise TypeError("complex taps for a filter created with real taps")
        t = np.ascontiguousarray(a, dtype=np.complex64 if self._complex else np.float32).reshape(-1)
        check(self._L.mi355_xlate_set_taps(self._h, _hp(t), int(t.size)), "mi355_xlate_set_taps")

    def bandpass_taps(self, channel=0):
        """the float32 band-pass taps b_c the kernels use"""
        n = self.ntaps()
        out = np.empty(n, np.complex64)
        check(min(self._L.mi355_xlate_get_bandpass_taps(self._h, int(channel), _hp(out), n), 0), "mi355_xlate_get_bandpass_taps")
        return out

    def center_freq(self, channel=0):
        f = C.c_double()
        check(self._L.mi355_xlate_get_center_freq(self._h, int(channel), C.byref(f)), "mi355_xlate_get_center_freq")
        return f.value

    def set_center_freq(self, freq, channel=0):
        """GNU Radio's set_center_freq(freq) for channel 0; the phase stays continuous"""
        check(self._L.mi355_xlate_set_center_freq(self._h, int(channel), float(freq)), "mi355_xlate_set_center_freq")

    def state(self, channel=0):
        """(phase, increment) of the channel's 64-bit accumulator as Python integers: the phase of the next output"""
        p, i = C.c_ulonglong(), C.c_ulonglong()
        check(self._L.mi355_xlate_get_state(self._h, int(channel), C.byref(p), C.byref(i)), "mi355_xlate_get_state")
        return p.value, i.value

    def set_phase(self, phase, channel=0):
        check(self._L.mi355_xlate_set_phase(self._h, int(channel), int(phase) % (1 << 64)), "mi355_xlate_set_phase")

    def skip(self, noutputs):
        """advance every channel's phase as if `noutputs` outputs had been made"""
        check(self._L.mi355_xlate_skip(self._h, int(noutputs)), "mi355_xlate_skip")

    def route(self):
        return self._L.mi355_xlate_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_xlate_set_generic(self._h, 1 if on else 0), "mi355_xlate_set_generic")

    def plan(self, noutput_items):
        """items of history-prefixed input a call of `noutput_items` outputs reads"""
        nin = C.c_longlong()
        check(self._L.mi355_xlate_plan(self._decim, self.ntaps(), int(noutput_items), C.byref(nin), None), "mi355_xlate_plan")
        return nin.value

    def work(self, noutput_items, input_items, output_items):
        """host buffers; input_items[0] is the history-prefixed buffer, output_items one complex64 array per channel"""
        n = int(noutput_items)
        if n == 0:
            return 0
        x = _host(input_items[0], np.complex64)
        need = self.plan(n)
        if x.size < need:
            raise ValueError("clFreqXlatingFIRFilter work(): need %d input items (history included), got %d" % (need, x.size))
        if len(output_items) != self._nch:
            raise ValueError("clFreqXlatingFIRFilter work(): %d channels, %d output buffers" % (self._nch, len(output_items)))
        ys = [_host(y, np.complex64, writable=True) for y in output_items]
        for y in ys:
            _need("output", y, n)
        ptrs = (C.c_void_p * self._nch)(*[y.ctypes.data for y in ys])
        check(self._L.mi355_xlate_work(self._h, n, _hp(x), ptrs), "mi355_xlate_work")
        return n

    def work_device(self, noutput_items, input_items, output_items):
        n = int(noutput_items)
        if n == 0:
            return 0
        if len(output_items) != self._nch:
            raise ValueError("clFreqXlatingFIRFilter work_device(): %d channels, %d output buffers" % (self._nch, len(output_items)))
        xin = _dp(input_items[0], self.plan(n) * 8, "input")
        ptrs = (C.c_void_p * self._nch)(*[_dp(y, n * 8, "output").value for y in output_items])
        check(self._L.mi355_xlate_work_dev(self._h, n, xin, ptrs, _torch_stream(self.device)), "mi355_xlate_work_dev")
        return n


BEAMFORM_VOLTAGE, BEAMFORM_POWER = 0, 1


class clBeamformer(_Block):
    """Tied-array beamformer on the X-engine's int8 frames (beyond the reference module; the contract is in include/mi355_clenabled.h):
    per channel and polarisation, `num_beams` weighted sums of the `num_inputs` stations with complex int8 weights, as voltage beams
    (complex64 holding exact integers, one unit = one frame) or as power integrated over `integration` frames (float32 of an exact
    int64 sum, one unit = one window; `stokes_i` adds the two polarisations).  `weights`: int8 in the layout [f][p][b][s]{re, im},
    components -127 .. 127, or None for all zero.  Every output is bit-exact on either route and for any split into calls."""
    _destroy = "mi355_beamform_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, mode, polarization, num_inputs, num_channels, num_beams,
                 integration=1, stokes_i=False, weights=None, setDebug=0):
        self.mode, self.npol = int(mode), int(polarization)
        self.num_inputs, self.num_channels, self.num_beams = int(num_inputs), int(num_channels), int(num_beams)
        self.integration, self.stokes_i = int(integration), 1 if stokes_i else 0
        L = lib()
        fb, fpu, ob = C.c_longlong(), C.c_int(), C.c_longlong()
        # argument errors before a context exists
        check(L.mi355_beamform_plan(self.mode, self.npol, self.num_inputs, self.num_channels, self.num_beams, self.integration, self.stokes_i,
                                    C.byref(fb), C.byref(fpu), C.byref(ob)), "mi355_beamform_plan")
        self._frame_bytes, self._fpu, self._out_bytes = fb.value, fpu.value, ob.value
        w = None if weights is None else self._weights(weights, self.weight_bytes())
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_beamform_create(self._ctx, self.mode, self.npol, self.num_inputs, self.num_channels, self.num_beams,
                                            self.integration, self.stokes_i, None if w is None else _hp(w), C.byref(self._h)),
              "mi355_beamform_create")

    @staticmethod
    def _weights(w, nbytes):
        a = np.ascontiguousarray(w)
        if a.dtype != np.int8:
            raise TypeError("weights are int8 {re, im} pairs")
        if a.size != nbytes:
            raise ValueError("weights hold %d bytes, the geometry needs %d" % (a.size, nbytes))
        return a

    def weight_bytes(self):
        return 2 * self.num_channels * self.npol * self.num_beams * self.num_inputs

    def frame_bytes(self):
        return self._frame_bytes

    def frames_per_unit(self):
        return self._fpu

    def out_bytes_per_unit(self):
        return self._out_bytes

    def out_items_per_unit(self):
        return self._out_bytes // (8 if self.mode == BEAMFORM_VOLTAGE else 4)

    def route(self):
        return self._L.mi355_beamform_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_beamform_set_generic(self._h, 1 if on else 0), "mi355_beamform_set_generic")

    def set_weights(self, weights):
        check(self._L.mi355_beamform_set_weights(self._h, _hp(self._weights(weights, self.weight_bytes()))), "mi355_beamform_set_weights")

    def set_beam_weights(self, beam, w_beam):
        """the weights of one beam, [f][p][s]{re, im}"""
        w = self._weights(w_beam, 2 * self.num_channels * self.npol * self.num_inputs)
        check(self._L.mi355_beamform_set_beam_weights(self._h, int(beam), _hp(w)), "mi355_beamform_set_beam_weights")

    def weights(self):
        out = np.empty((self.num_channels, self.npol, self.num_beams, self.num_inputs, 2), np.int8)
        check(self._L.mi355_beamform_get_weights(self._h, _hp(out), out.nbytes), "mi355_beamform_get_weights")
        return out

    def _out_dtype(self):
        return np.complex64 if self.mode == BEAMFORM_VOLTAGE else np.float32

    def work(self, nunits, input_items, output_items):
        """host buffers: input_items[0] int8 frames (nunits * frames_per_unit of them), output_items[0] complex64 / float32"""
        n = int(nunits)
        if n == 0:
            return 0
        x = _host(input_items[0])
        if x.nbytes < n * self._fpu * self._frame_bytes:
            raise ValueError("clBeamformer work(): need %d input bytes, got %d" % (n * self._fpu * self._frame_bytes, x.nbytes))
        y = _host(output_items[0], self._out_dtype(), writable=True)
        _need("output", y, n * self.out_items_per_unit())
        check(self._L.mi355_beamform_work(self._h, n, _hp(x), _hp(y)), "mi355_beamform_work")
        return n

    def work_device(self, nunits, input_items, output_items):
        n = int(nunits)
        if n == 0:
            return 0
        check(self._L.mi355_beamform_work_dev(self._h, n, _dp(input_items[0], n * self._fpu * self._frame_bytes, "input"),
                                              _dp(output_items[0], n * self._out_bytes, "output"), _torch_stream(self.device)),
              "mi355_beamform_work_dev")
        return n


class clFEngine(_Block):
    """F-engine in front of clXEngine / clBeamformer (beyond the reference module; the contract is in include/mi355_clenabled.h):
    `num_inputs` stations of `polarization` complex64 streams each (input r = s * npol + p) go through a critically sampled polyphase
    filter bank (`taps`: P * num_channels real prototype taps, None = all ones; P = 1 is a windowed FFT), a forward DFT, a real gain
    per (input, channel) and symmetric int8 quantisation (round half to even, -127 .. 127, NaN -> 0) into the frames
    [t][station][chan][pol]{I, Q}.  Every saturated or NaN component is counted per input (`clips()`).  Every input buffer is
    history-prefixed: it starts at the first item of the first frame's window and holds (n + P - 1) * num_channels items."""
    _destroy = "mi355_fengine_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, polarization, num_inputs, num_channels, taps=None,
                 taps_per_channel=1, shift=False, gains=None, setDebug=0):
        self.npol, self.num_inputs, self.num_channels = int(polarization), int(num_inputs), int(num_channels)
        self.taps_per_channel, self.shift = int(taps_per_channel), 1 if shift else 0
        L = lib()
        fb, hi = C.c_longlong(), C.c_longlong()
        # argument errors before a context exists
        check(L.mi355_fengine_plan(self.num_inputs, self.npol, self.num_channels, self.taps_per_channel, self.shift, 0, C.byref(fb),
                                   C.byref(hi), None), "mi355_fengine_plan")
        self._frame_bytes, self._history = fb.value, hi.value
        self._nin = self.num_inputs * self.npol
        t = None
        if taps is not None:
            t = np.ascontiguousarray(taps, np.float32)
            if t.size != self.taps_per_channel * self.num_channels:
                raise ValueError("taps hold %d values, the geometry needs %d" % (t.size, self.taps_per_channel * self.num_channels))
        g = None if gains is None else self._gains(gains, self._nin * self.num_channels)
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_fengine_create(self._ctx, self.num_inputs, self.npol, self.num_channels, self.taps_per_channel,
                                           None if t is None else _hp(t), self.shift, None if g is None else _hp(g), C.byref(self._h)),
              "mi355_fengine_create")

    @staticmethod
    def _gains(g, n):
        a = np.ascontiguousarray(g, np.float32)
        if a.size != n:
            raise ValueError("gains hold %d values, the geometry needs %d" % (a.size, n))
        return a

    def frame_bytes(self):
        return self._frame_bytes

    def history_items(self):
        """items in front of a call's first new frame: (P - 1) * num_channels (the GR block's history() is this plus one)"""
        return self._history

    def items_per_input(self, nframes):
        return 0 if nframes == 0 else int(nframes) * self.num_channels + self._history

    def route(self):
        return self._L.mi355_fengine_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_fengine_set_generic(self._h, 1 if on else 0), "mi355_fengine_set_generic")

    def set_gains(self, gains):
        check(self._L.mi355_fengine_set_gains(self._h, _hp(self._gains(gains, self._nin * self.num_channels))), "mi355_fengine_set_gains")

    def set_input_gain(self, r, gain):
        check(self._L.mi355_fengine_set_input_gain(self._h, int(r), _hp(self._gains(gain, self.num_channels))), "mi355_fengine_set_input_gain")

    def gains(self):
        out = np.empty((self._nin, self.num_channels), np.float32)
        check(self._L.mi355_fengine_get_gains(self._h, _hp(out), out.size), "mi355_fengine_get_gains")
        return out

    def clips(self, reset=False):
        """saturated or NaN components per input so far (waits for the device)"""
        out = np.zeros(self._nin, np.uint64)
        check(self._L.mi355_fengine_get_clips(self._h, _hp(out), 1 if reset else 0), "mi355_fengine_get_clips")
        return out

    def work(self, nframes, input_items, output_items):
        """host buffers: one history-prefixed complex64 array per input, output_items[0] int8 / uint8 frames"""
        n = int(nframes)
        if n == 0:
            return 0
        if len(input_items) != self._nin:
            raise ValueError("clFEngine work(): %d inputs, %d buffers" % (self._nin, len(input_items)))
        xs = [_host(x, np.complex64) for x in input_items]
        for x in xs:
            if x.size < self.items_per_input(n):
                raise ValueError("clFEngine work(): need %d input items (history included), got %d" % (self.items_per_input(n), x.size))
        y = _host(output_items[0], writable=True)
        if y.nbytes < n * self._frame_bytes:
            raise ValueError("clFEngine work(): output holds %d bytes, the call needs %d" % (y.nbytes, n * self._frame_bytes))
        ptrs = (C.c_void_p * self._nin)(*[x.ctypes.data for x in xs])
        check(self._L.mi355_fengine_work(self._h, n, ptrs, _hp(y)), "mi355_fengine_work")
        return n

    def work_device(self, nframes, input_items, output_items):
        n = int(nframes)
        if n == 0:
            return 0
        if len(input_items) != self._nin:
            raise ValueError("clFEngine work_device(): %d inputs, %d buffers" % (self._nin, len(input_items)))
        ptrs = (C.c_void_p * self._nin)(*[_dp(x, self.items_per_input(n) * 8, "input").value for x in input_items])
        check(self._L.mi355_fengine_work_dev(self._h, n, ptrs, _dp(output_items[0], n * self._frame_bytes, "output"),
                                             _torch_stream(self.device)), "mi355_fengine_work_dev")
        return n


DEDISP_TRIAL_MAJOR, DEDISP_TIME_MAJOR = 0, 1


def dedisp_delays(f0_mhz, df_mhz, num_channels, tsamp_s, dm):
    """(delay[d][f] int32, max_delay): the cold-plasma delay table of mi355_dedisp_delays for a band of `num_channels` channels
    nu_f = f0 + f df MHz against its highest frequency, dispersion measures `dm` in pc cm^-3 and a sampling time in seconds"""
    dms = np.ascontiguousarray(dm, np.float64).reshape(-1)
    out = np.empty((dms.size, int(num_channels)), np.int32)
    top = C.c_int()
    check(lib().mi355_dedisp_delays(float(f0_mhz), float(df_mhz), int(num_channels), float(tsamp_s), _hp(dms), dms.size, _hp(out), C.byref(top)),
          "mi355_dedisp_delays")
    return out, top.value


class clDedisperser(_Block):
    """Exact incoherent dedispersion behind clBeamformer's POWER output (beyond the reference module; the contract is in
    include/mi355_clenabled.h): x[t][row][chan] float32 summed over the channels at per-(trial, channel) sample delays,
    y(r, d, t) = sum_f x[t + delay[d][f]][r][f] in ascending channel order, one binary32 rounding per addition, -1 entries skipped.
    `delays`: int32 [num_trials][num_channels], each 0 .. max_delay or -1, None for all zero.  A call for n outputs reads n + max_delay
    samples.  Output TIME_MAJOR y[t][r][d], or TRIAL_MAJOR y[(r D + d) out_pitch + t].  Bit-exact on either route and for any split."""
    _destroy = "mi355_dedisp_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, num_trials, max_delay,
                 order=DEDISP_TIME_MAJOR, delays=None, setDebug=0):
        self.num_rows, self.num_channels, self.num_trials = int(num_rows), int(num_channels), int(num_trials)
        self.max_delay, self.order = int(max_delay), int(order)
        L = lib()
        fi, hi, fo = C.c_longlong(), C.c_longlong(), C.c_longlong()
        # argument errors before a context exists
        check(L.mi355_dedisp_plan(self.num_rows, self.num_channels, self.num_trials, self.max_delay, self.order, C.byref(fi), C.byref(hi),
                                  C.byref(fo)), "mi355_dedisp_plan")
        self._in_floats, self._history, self._out_floats = fi.value, hi.value, fo.value
        t = None if delays is None else self._table(delays)
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_dedisp_create(self._ctx, self.num_rows, self.num_channels, self.num_trials, self.max_delay, self.order,
                                          None if t is None else _hp(t), C.byref(self._h)), "mi355_dedisp_create")

    def _table(self, delays):
        a = np.ascontiguousarray(delays)
        if a.dtype != np.int32:
            raise TypeError("delays are int32")
        if a.size != self.num_trials * self.num_channels:
            raise ValueError("delays hold %d entries, the geometry needs %d" % (a.size, self.num_trials * self.num_channels))
        return a

    def in_floats_per_sample(self):
        return self._in_floats

    def out_floats_per_sample(self):
        return self._out_floats

    def history(self):
        """samples of look-ahead behind a call's last output: max_delay (the GR block's history() is this plus one)"""
        return self._history

    def in_floats(self, n):
        return 0 if n == 0 else (int(n) + self._history) * self._in_floats

    def out_floats(self, n, out_pitch=None):
        """floats from the first to one past the last a call for n outputs writes"""
        if n == 0:
            return 0
        if self.order == DEDISP_TIME_MAJOR:
            return int(n) * self._out_floats
        return (self._out_floats - 1) * (int(n) if out_pitch is None else int(out_pitch)) + int(n)

    def route(self):
        return self._L.mi355_dedisp_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_dedisp_set_generic(self._h, 1 if on else 0), "mi355_dedisp_set_generic")

    def set_delays(self, delays):
        check(self._L.mi355_dedisp_set_delays(self._h, _hp(self._table(delays))), "mi355_dedisp_set_delays")

    def delays(self):
        out = np.empty((self.num_trials, self.num_channels), np.int32)
        check(self._L.mi355_dedisp_get_delays(self._h, _hp(out), out.size), "mi355_dedisp_get_delays")
        return out

    def _pitch(self, n, out_pitch):
        if self.order == DEDISP_TIME_MAJOR:
            return 0 if out_pitch is None else int(out_pitch)
        return n if out_pitch is None else int(out_pitch)

    def work(self, noutput_items, input_items, output_items, out_pitch=None):
        """host buffers: input_items[0] float32 [n + max_delay][R][F], output_items[0] float32; out_pitch (TRIAL_MAJOR): floats between
        the time series, default n"""
        n = int(noutput_items)
        if n == 0:
            return 0
        x = _host(input_items[0], np.float32)
        _need("input", x, self.in_floats(n))
        y = _host(output_items[0], np.float32, writable=True)
        pitch = self._pitch(n, out_pitch)
        if self.order == DEDISP_TRIAL_MAJOR and pitch >= n:
            _need("output", y, self.out_floats(n, pitch))
        elif self.order == DEDISP_TIME_MAJOR:
            _need("output", y, self.out_floats(n))
        check(self._L.mi355_dedisp_work(self._h, n, _hp(x), _hp(y), pitch), "mi355_dedisp_work")
        return n

    def work_device(self, noutput_items, input_items, output_items, out_pitch=None):
        n = int(noutput_items)
        if n == 0:
            return 0
        pitch = self._pitch(n, out_pitch)
        need = self.out_floats(n, pitch) if (self.order == DEDISP_TRIAL_MAJOR and pitch >= n) else self.out_floats(n)
        check(self._L.mi355_dedisp_work_dev(self._h, n, _dp(input_items[0], self.in_floats(n) * 4, "input"),
                                            _dp(output_items[0], need * 4, "output"), pitch, _torch_stream(self.device)),
              "mi355_dedisp_work_dev")
        return n


PSEARCH_TRIAL_MAJOR, PSEARCH_TIME_MAJOR = 0, 1
PSEARCH_PEAK = np.dtype([("snr", np.float32), ("loc", np.uint32)])
PSEARCH_CAND = np.dtype([("snr", np.float32), ("loc", np.uint32), ("series", np.uint32), ("block", np.uint32)])


class _PeakSearch(_Block):
    """what clPulseSearch, clPeriodSearch and clSpectralSearch share: the check of a per-series statistic, the view of the peak records
    and the candidate buffers of the last call"""
    _series_of = "block"     # "... the block has N series"
    _cands = _counts = None  # the candidate buffers of the last call: numpy (work) or CUDA tensors (work_device)

    def _per_series(self, a, name="inv_sigma"):
        a = np.ascontiguousarray(a)
        if a.dtype != np.float32:
            raise TypeError("%s is float32" % name)
        if a.size != self.num_series:
            raise ValueError("%s holds %d entries, the %s has %d series" % (name, a.size, self._series_of, self.num_series))
        return a

    def _new_cands(self, like=None):
        """(candidate buffer, counters) of the block's own for a call, (None, None) with max_cands = 0: numpy, or torch on like's device"""
        if not self.max_cands:
            return None, None
        if like is None:
            return np.zeros(self.max_cands, PSEARCH_CAND), np.zeros(2, np.uint32)
        import torch
        return (torch.empty(self.max_cands * 4, dtype=torch.int32, device=like.device),
                torch.empty(2, dtype=torch.int32, device=like.device))

    @staticmethod
    def peaks_of(t):
        """the records of a work_device output tensor as a flat PSEARCH_PEAK array on the host (waits for the tensor's device)"""
        return np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1).view(np.uint8).view(PSEARCH_PEAK)

    def candidates(self):
        """(records, found) of the last work() / work_device() call: a PSEARCH_CAND array of the min(found, max_cands) stored records in
        no particular order, and the number found; waits for the device after a work_device() call"""
        if self._cands is None:
            return np.zeros(0, PSEARCH_CAND), 0
        if isinstance(self._cands, np.ndarray):
            cands, counts = self._cands, self._counts
        else:
            counts = self._counts.detach().cpu().numpy().reshape(-1).view(np.uint8).view(np.uint32)
            cands = np.ascontiguousarray(self._cands.detach().cpu().numpy()).reshape(-1).view(np.uint8).view(PSEARCH_CAND)
        return cands[:int(counts[1])].copy(), int(counts[0])


class clPulseSearch(_PeakSearch):
    """Exact boxcar single-pulse search behind clDedisperser (beyond the reference module; the contract is in
    include/mi355_clenabled.h): per series K boxcars of widths 2^0 .. 2^(K-1) summed as a fixed dyadic tree of binary32 additions,
    snr_k[t] = (b_k[t] - mean 2^k) (inv_sigma c_k), and per (block of block_len outputs, series) the record {snr, loc = (k << 24) | t}
    of the largest one (ties: smallest k, then smallest t; NaN never takes part).  A call for `nblocks` blocks reads
    nblocks block_len + history() samples per series: TIME_MAJOR x[t][r][d], or TRIAL_MAJOR x[(r D + d) in_pitch + t].  With
    max_cands > 0 every peak at or above the threshold (set_threshold, +Inf at first) is also listed: candidates().  Bit-exact on
    either route, for any split into calls and any alignment."""
    _destroy = "mi355_psearch_destroy"
    _series_of = "geometry"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, num_rows, num_trials, num_widths, block_len,
                 order=PSEARCH_TIME_MAJOR, mean=None, inv_sigma=None, max_cands=0, setDebug=0):
        self.num_rows, self.num_trials, self.num_widths = int(num_rows), int(num_trials), int(num_widths)
        self.block_len, self.order, self.max_cands = int(block_len), int(order), int(max_cands)
        L = lib()
        fi, hi, pb = C.c_longlong(), C.c_longlong(), C.c_longlong()
        # argument errors before a context exists
        check(L.mi355_psearch_plan(self.num_rows, self.num_trials, self.num_widths, self.block_len, self.order, C.byref(fi), C.byref(hi),
                                   C.byref(pb)), "mi355_psearch_plan")
        if self.max_cands < 0:
            raise ValueError("max_cands is negative")
        self.num_series, self._history = fi.value, hi.value
        m = None if mean is None else self._per_series(mean, "mean")
        g = None if inv_sigma is None else self._per_series(inv_sigma, "inv_sigma")
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_psearch_create(self._ctx, self.num_rows, self.num_trials, self.num_widths, self.block_len, self.order,
                                           None if m is None else _hp(m), None if g is None else _hp(g), C.byref(self._h)),
              "mi355_psearch_create")

    def history(self):
        """samples of look-ahead behind a call's last output: 2^(K-1) - 1 (the GR block's history() is this plus one)"""
        return self._history

    def in_floats(self, nblocks, in_pitch=None):
        """floats from the first to one past the last a call for nblocks blocks reads"""
        if nblocks == 0:
            return 0
        rows = int(nblocks) * self.block_len + self._history
        if self.order == PSEARCH_TIME_MAJOR:
            return rows * self.num_series
        return (self.num_series - 1) * (rows if in_pitch is None else int(in_pitch)) + rows

    def route(self):
        return self._L.mi355_psearch_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_psearch_set_generic(self._h, 1 if on else 0), "mi355_psearch_set_generic")

    def set_threshold(self, threshold):
        check(self._L.mi355_psearch_set_threshold(self._h, float(threshold)), "mi355_psearch_set_threshold")

    def set_stats(self, mean, inv_sigma):
        check(self._L.mi355_psearch_set_stats(self._h, _hp(self._per_series(mean, "mean")), _hp(self._per_series(inv_sigma, "inv_sigma"))),
              "mi355_psearch_set_stats")

    def stats(self):
        m, g = np.empty(self.num_series, np.float32), np.empty(self.num_series, np.float32)
        check(self._L.mi355_psearch_get_stats(self._h, _hp(m), _hp(g), self.num_series), "mi355_psearch_get_stats")
        return m, g

    def measure(self, x, n, in_pitch=None):
        """(mean, inv_sigma) of n samples per series of `x` (numpy, or a CUDA tensor) in the block's order, computed in float64; the
        values are not installed: pass them to set_stats()"""
        n = int(n)
        pitch = 0 if self.order == PSEARCH_TIME_MAJOR else (n if in_pitch is None else int(in_pitch))
        need = n * self.num_series if self.order == PSEARCH_TIME_MAJOR else (self.num_series - 1) * pitch + n
        m, g = np.empty(self.num_series, np.float32), np.empty(self.num_series, np.float32)
        if isinstance(x, np.ndarray):
            x = _host(x, np.float32)
            _need("input", x, need)
            p, dev = _hp(x), 0
        else:
            p, dev = _dp(x, need * 4, "input"), 1
        check(self._L.mi355_psearch_measure(self._h, n, p, pitch, dev, _hp(m), _hp(g)), "mi355_psearch_measure")
        return m, g

    def _pitch(self, nblocks, in_pitch):
        if self.order == PSEARCH_TIME_MAJOR:
            return 0 if in_pitch is None else int(in_pitch)
        return nblocks * self.block_len + self._history if in_pitch is None else int(in_pitch)

    def work(self, noutput_items, input_items, output_items, in_pitch=None):
        """host buffers: input_items[0] float32; output_items[0] a PSEARCH_PEAK array of noutput_items (blocks) x R x D records"""
        nb = int(noutput_items)
        if nb == 0:
            return 0
        x = _host(input_items[0], np.float32)
        pitch = self._pitch(nb, in_pitch)
        if self.order == PSEARCH_TIME_MAJOR or pitch >= nb * self.block_len + self._history:
            _need("input", x, self.in_floats(nb, pitch))
        y = _host(output_items[0], PSEARCH_PEAK, writable=True)
        _need("output", y, nb * self.num_series)
        cands, counts = self._new_cands()
        check(self._L.mi355_psearch_work(self._h, nb * self.block_len, _hp(x), pitch, _hp(y), None if cands is None else _hp(cands),
                                         self.max_cands, None if counts is None else _hp(counts)), "mi355_psearch_work")
        self._cands, self._counts = cands, counts
        return nb

    def work_device(self, noutput_items, input_items, output_items, in_pitch=None):
        """CUDA tensors: output_items[0] holds 8 bytes per record (torch.int64, say; see peaks_of); output_items[1:3], if given, are
        the candidate buffer (16 max_cands bytes) and the two 32-bit counters, otherwise the block keeps its own"""
        nb = int(noutput_items)
        if nb == 0:
            return 0
        pitch = self._pitch(nb, in_pitch)
        ok = self.order == PSEARCH_TIME_MAJOR or pitch >= nb * self.block_len + self._history
        xin = _dp(input_items[0], self.in_floats(nb, pitch) * 4 if ok else None, "input")
        if self.max_cands and len(output_items) >= 3:
            cands, counts = output_items[1], output_items[2]
        else:
            cands, counts = self._new_cands(input_items[0])
        check(self._L.mi355_psearch_work_dev(self._h, nb * self.block_len, xin, pitch, _dp(output_items[0], nb * self.num_series * 8, "output"),
                                             None if cands is None else _dp(cands, self.max_cands * 16, "candidates"), self.max_cands,
                                             None if counts is None else _dp(counts, 8, "counts"), _torch_stream(self.device)),
              "mi355_psearch_work_dev")
        self._cands, self._counts = cands, counts
        return nb

    def search(self, x, nblocks, in_pitch=None):
        """work() on a numpy input: the peaks as a PSEARCH_PEAK array [nblocks][R][D]"""
        y = np.empty((int(nblocks), self.num_rows, self.num_trials), PSEARCH_PEAK)
        self.work(nblocks, [x], [y], in_pitch)
        return y

def sk_estimate(x, nd, stride=1):
    """the spectral-kurtosis estimator of clFilterbankCleaner (mi355_fbclean_sk_estimate, host only) on one column of float32 samples
    x[0], x[stride], ...: block_len = the number of samples of the column, a multiple of 16 in 16 .. 4096"""
    a = _host(x, np.float32).reshape(-1)
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be >= 1")
    sk = C.c_double()
    check(lib().mi355_fbclean_sk_estimate(_hp(a), (a.size + stride - 1) // stride, stride, float(nd), C.byref(sk)), "mi355_fbclean_sk_estimate")
    return sk.value


class clFilterbankCleaner(_Block):
    """Exact RFI excision between clBeamformer's POWER output and clDedisperser (beyond the reference module; the contract is in
    include/mi355_clenabled.h): per (block of block_len samples, row, channel) float64 mean, variance and spectral kurtosis in a pinned
    order, a channel flag (mask, var > 0, sk_lo <= sk <= sk_hi), y = (x - m32) is32 for the good channels and +0 for the flagged ones,
    and with zero_dm the mean over the good channels removed per time sample, time samples with zs^2 > td^2 ng zeroed.  x[t][r][f]
    float32 in, the same layout out; the flags and {m32, is32} are optional outputs.  Bit-exact on either route, for any split into
    calls at block boundaries and any alignment; in place when input and output are the same buffer."""
    _destroy = "mi355_fbclean_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, block_len, nd=1.0, sk_lo=-np.inf,
                 sk_hi=np.inf, td=np.inf, zero_dm=0, mask=None, setDebug=0):
        self.num_rows, self.num_channels, self.block_len = int(num_rows), int(num_channels), int(block_len)
        L = lib()
        fs, cb, tb = C.c_longlong(), C.c_longlong(), C.c_longlong()
        # argument errors before a context exists
        check(L.mi355_fbclean_plan(self.num_rows, self.num_channels, self.block_len, C.byref(fs), C.byref(cb), C.byref(tb)), "mi355_fbclean_plan")
        self._floats = fs.value
        m = None if mask is None else self._mask(mask)
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_fbclean_create(self._ctx, self.num_rows, self.num_channels, self.block_len, float(nd), float(sk_lo), float(sk_hi),
                                           float(td), int(zero_dm), None if m is None else _hp(m), C.byref(self._h)), "mi355_fbclean_create")

    def _mask(self, mask):
        a = np.ascontiguousarray(mask)
        if a.dtype != np.uint8:
            raise TypeError("mask is uint8")
        if a.size != self.num_channels:
            raise ValueError("mask holds %d entries, the geometry has %d channels" % (a.size, self.num_channels))
        return a

    def floats_per_sample(self):
        return self._floats

    def route(self):
        return self._L.mi355_fbclean_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_fbclean_set_generic(self._h, 1 if on else 0), "mi355_fbclean_set_generic")

    def set_limits(self, nd, sk_lo, sk_hi, td, zero_dm):
        check(self._L.mi355_fbclean_set_limits(self._h, float(nd), float(sk_lo), float(sk_hi), float(td), int(zero_dm)), "mi355_fbclean_set_limits")

    def limits(self):
        """(nd, sk_lo, sk_hi, td, zero_dm)"""
        v = [C.c_double() for _ in range(4)]
        z = C.c_int()
        check(self._L.mi355_fbclean_get_limits(self._h, *[C.byref(a) for a in v], C.byref(z)), "mi355_fbclean_get_limits")
        return tuple(a.value for a in v) + (z.value,)

    def set_mask(self, mask):
        check(self._L.mi355_fbclean_set_mask(self._h, _hp(self._mask(mask))), "mi355_fbclean_set_mask")

    def mask(self):
        out = np.empty(self.num_channels, np.uint8)
        check(self._L.mi355_fbclean_get_mask(self._h, _hp(out), out.size), "mi355_fbclean_get_mask")
        return out

    sk_estimate = staticmethod(sk_estimate)

    def work(self, noutput_items, input_items, output_items):
        """host buffers: noutput_items time samples, a multiple of block_len.  input_items[0] float32 [n][R][F]; output_items[0] the
        same (it may be the input array: in place); output_items[1:4], each optional or None: cflags uint8 [n / block_len][R][F],
        tflags uint8 [n][R], stats float32 [n / block_len][R][F][2]"""
        n = int(noutput_items)
        if n == 0:
            return 0
        nb = n // self.block_len
        x = _host(input_items[0], np.float32)
        _need("input", x, n * self._floats)
        y = _host(output_items[0], np.float32, writable=True)
        _need("output", y, n * self._floats)
        opt = [None, None, None]
        for k, (dtype, items) in enumerate(((np.uint8, nb * self._floats), (np.uint8, n * self.num_rows), (np.float32, 2 * nb * self._floats))):
            if len(output_items) > k + 1 and output_items[k + 1] is not None:
                opt[k] = _host(output_items[k + 1], dtype, writable=True)
                _need("output %d" % (k + 1), opt[k], items)
        check(self._L.mi355_fbclean_work(self._h, n, _hp(x), _hp(y), *[None if a is None else _hp(a) for a in opt]), "mi355_fbclean_work")
        return n

    def work_device(self, noutput_items, input_items, output_items):
        """CUDA tensors, enqueue only on torch's current stream; the same buffers as work()"""
        n = int(noutput_items)
        if n == 0:
            return 0
        nb = n // self.block_len
        opt = [None, None, None]
        for k, nbytes in enumerate((nb * self._floats, n * self.num_rows, 8 * nb * self._floats)):
            if len(output_items) > k + 1 and output_items[k + 1] is not None:
                opt[k] = _dp(output_items[k + 1], nbytes, "output %d" % (k + 1))
        check(self._L.mi355_fbclean_work_dev(self._h, n, _dp(input_items[0], n * self._floats * 4, "input"),
                                             _dp(output_items[0], n * self._floats * 4, "output"), *opt, _torch_stream(self.device)),
              "mi355_fbclean_work_dev")
        return n

    def clean(self, x, flags=False):
        """work() on a numpy input [n][R][F]: the cleaned filterbank, or with flags (out, cflags, tflags, stats)"""
        x = _host(x, np.float32)
        n = x.size // self._floats
        nb = n // self.block_len
        y = np.empty((n, self.num_rows, self.num_channels), np.float32)
        if not flags:
            self.work(n, [x], [y])
            return y
        cf = np.empty((nb, self.num_rows, self.num_channels), np.uint8)
        tf = np.empty((n, self.num_rows), np.uint8)
        st = np.empty((nb, self.num_rows, self.num_channels, 2), np.float32)
        self.work(n, [x], [y, cf, tf, st])
        return y, cf, tf, st


def fold_model(period_s, pdot, tsamp_s, phase0_turns=0.0):
    """the three uint64 words {phi0, nu, nudot} of clFolder's phase model (mi355_fold_model, host only, computed in long double): a
    pulsar of period `period_s` seconds and period derivative `pdot` sampled every `tsamp_s` seconds, at `phase0_turns` at sample 0"""
    out = np.empty(3, np.uint64)
    check(lib().mi355_fold_model(float(period_s), float(pdot), float(tsamp_s), float(phase0_turns), _hp(out)), "mi355_fold_model")
    return out


def fold_bins(model, T0, n, nbin):
    """bin(T) of T = T0 .. T0 + n - 1 for one model of three uint64 words, bit for bit as clFolder computes it (mi355_fold_bins, host
    only): int32 [n]"""
    m = np.ascontiguousarray(model, np.uint64).reshape(-1)
    if m.size != 3:
        raise ValueError("a model is three 64-bit words")
    out = np.empty(max(int(n), 0), np.int32)
    check(lib().mi355_fold_bins(_hp(m), int(T0) & 0xFFFFFFFFFFFFFFFF, int(n), int(nbin), _hp(out)), "mi355_fold_bins")
    return out


class clFolder(_Block):
    """Exact pulsar folding behind clBeamformer's POWER output and clFilterbankCleaner (beyond the reference module; the contract is in
    include/mi355_clenabled.h): x[t][r][f] float32, optionally with the cleaner's tflags[t][r], folded modulo a per-row integer phase
    model {phi0, nu, nudot} (units of 2^-64 turn) into out[j][r][b][f] per sub-integration of subint_len samples, each sum in ascending
    time with one binary32 rounding per addition, and optionally hits[j][r][b] uint32.  The handle counts the absolute sample index.
    Bit-exact on either route, for any split into calls at sub-integration boundaries and any alignment."""
    _destroy = "mi355_fold_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, nbin, subint_len, models, setDebug=0):
        self.num_rows, self.num_channels, self.nbin, self.subint_len = int(num_rows), int(num_channels), int(nbin), int(subint_len)
        L = lib()
        fs, fo, hs = C.c_longlong(), C.c_longlong(), C.c_longlong()
        # argument errors before a context exists
        check(L.mi355_fold_plan(self.num_rows, self.num_channels, self.nbin, self.subint_len, C.byref(fs), C.byref(fo), C.byref(hs)), "mi355_fold_plan")
        self._floats, self._out_floats, self._hits = fs.value, fo.value, hs.value
        m = self._models(models)
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_fold_create(self._ctx, self.num_rows, self.num_channels, self.nbin, self.subint_len, _hp(m), C.byref(self._h)),
              "mi355_fold_create")

    def _models(self, models):
        a = np.ascontiguousarray(models)
        if a.dtype != np.uint64:
            raise TypeError("models are uint64 words (nudot as two's complement)")
        if a.size != 3 * self.num_rows:
            raise ValueError("models hold %d words, the geometry has %d rows of 3" % (a.size, self.num_rows))
        return a

    def floats_per_sample(self):
        return self._floats

    def floats_per_subint(self):
        return self._out_floats

    def hits_per_subint(self):
        return self._hits

    def route(self):
        return self._L.mi355_fold_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_fold_set_generic(self._h, 1 if on else 0), "mi355_fold_set_generic")

    def set_models(self, models):
        check(self._L.mi355_fold_set_models(self._h, _hp(self._models(models))), "mi355_fold_set_models")

    def models(self):
        out = np.empty((self.num_rows, 3), np.uint64)
        check(self._L.mi355_fold_get_models(self._h, _hp(out), out.size), "mi355_fold_get_models")
        return out

    def sample(self):
        """the absolute index of the next sample"""
        t = C.c_ulonglong()
        check(self._L.mi355_fold_sample(self._h, C.byref(t)), "mi355_fold_sample")
        return t.value

    def set_sample(self, T):
        check(self._L.mi355_fold_set_sample(self._h, int(T) & 0xFFFFFFFFFFFFFFFF), "mi355_fold_set_sample")

    def skip(self, n):
        check(self._L.mi355_fold_skip(self._h, int(n)), "mi355_fold_skip")

    fold_model = staticmethod(fold_model)
    fold_bins = staticmethod(fold_bins)

    def work(self, noutput_items, input_items, output_items):
        """host buffers: noutput_items sub-integrations.  input_items[0] float32 [n subint_len][R][F]; input_items[1], optional or None:
        tflags uint8 [n subint_len][R]; output_items[0] float32 [n][R][nbin][F]; output_items[1], optional or None: hits uint32
        [n][R][nbin]"""
        ns = int(noutput_items)
        if ns == 0:
            return 0
        n = ns * self.subint_len
        x = _host(input_items[0], np.float32)
        _need("input", x, n * self._floats)
        tf = None
        if len(input_items) > 1 and input_items[1] is not None:
            tf = _host(input_items[1], np.uint8)
            _need("input 1", tf, n * self.num_rows)
        y = _host(output_items[0], np.float32, writable=True)
        _need("output", y, ns * self._out_floats)
        hits = None
        if len(output_items) > 1 and output_items[1] is not None:
            hits = _host(output_items[1], np.uint32, writable=True)
            _need("output 1", hits, ns * self._hits)
        check(self._L.mi355_fold_work(self._h, n, _hp(x), None if tf is None else _hp(tf), _hp(y), None if hits is None else _hp(hits)),
              "mi355_fold_work")
        return ns

    def work_device(self, noutput_items, input_items, output_items):
        """CUDA tensors, enqueue only on torch's current stream; the same buffers as work()"""
        ns = int(noutput_items)
        if ns == 0:
            return 0
        n = ns * self.subint_len
        tf = hits = None
        if len(input_items) > 1 and input_items[1] is not None:
            tf = _dp(input_items[1], n * self.num_rows, "input 1")
        if len(output_items) > 1 and output_items[1] is not None:
            hits = _dp(output_items[1], 4 * ns * self._hits, "output 1")
        check(self._L.mi355_fold_work_dev(self._h, n, _dp(input_items[0], n * self._floats * 4, "input"), tf,
                                          _dp(output_items[0], ns * self._out_floats * 4, "output"), hits, _torch_stream(self.device)),
              "mi355_fold_work_dev")
        return ns

    def fold(self, x, tflags=None, hits=False):
        """work() on a numpy input [n][R][F]: the archive [n / subint_len][R][nbin][F], or with hits (archive, hits)"""
        x = _host(x, np.float32)
        ns = x.size // self._floats // self.subint_len
        y = np.empty((ns, self.num_rows, self.nbin, self.num_channels), np.float32)
        if not hits:
            self.work(ns, [x, tflags], [y])
            return y
        h = np.empty((ns, self.num_rows, self.nbin), np.uint32)
        self.work(ns, [x, tflags], [y, h])
        return y, h


FFA_PEAK = PSEARCH_PEAK


def ffa_shift(log2_rows, i, r):
    """sh(i, r) of clPeriodSearch (mi355_ffa_shift, host only): the bins by which row r is read ahead in the profile of trial i"""
    v = lib().mi355_ffa_shift(int(log2_rows), int(i), int(r))
    if v < 0:
        raise ValueError("ffa_shift: log2_rows is 1 .. 12 and i, r lie below 2^log2_rows")
    return int(v)


def ffa_period(p, log2_rows, i, tsamp_s):
    """the period in seconds of trial (p, i) of clPeriodSearch (mi355_ffa_period, host only): (p + i / (2^log2_rows - 1)) tsamp_s, what
    fold_model() takes"""
    v = lib().mi355_ffa_period(int(p), int(log2_rows), int(i), float(tsamp_s))
    if v != v:
        raise ValueError("ffa_period: an argument outside the block's ranges")
    return v


class clPeriodSearch(_PeakSearch):
    """Exact fast-folding search for unknown periods behind clDedisperser's per-trial output (beyond the reference module; the contract
    is in include/mi355_clenabled.h).  For every series s and base period p_lo <= p <= p_hi the first 2^L p samples are 2^L rows of p
    bins, combined by the FFA's fixed tree of binary32 additions into 2^L profiles, the trial periods p + i / (2^L - 1) samples.  Every
    profile is searched with K circular dyadic boxcars, snr_k[j] = (b_k[j] - mean 2^(L+k)) (inv_sigma c_(L+k)), and gives the record
    {snr, loc = (k << 24) | j} of its largest value (ties: smallest k, then smallest j; NaN never takes part): peaks[s][p - p_lo][i].
    Optionally the profiles themselves, [s][p - p_lo][i][p_hi].  Bit-exact on either route and for any alignment and pitch."""
    _destroy = "mi355_ffa_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, num_series, p_lo, p_hi, log2_rows, num_widths, mean=None,
                 inv_sigma=None, setDebug=0):
        self.num_series, self.p_lo, self.p_hi = int(num_series), int(p_lo), int(p_hi)
        self.log2_rows, self.num_widths = int(log2_rows), int(num_widths)
        # argument errors before a context exists
        self.N, self.records, self.profile_floats, self.scratch_bytes = self.plan(self.num_series, self.p_lo, self.p_hi, self.log2_rows,
                                                                                  self.num_widths)
        self.num_periods, self.num_rows = self.p_hi - self.p_lo + 1, 1 << self.log2_rows
        m = None if mean is None else self._per_series(mean, "mean")
        g = None if inv_sigma is None else self._per_series(inv_sigma, "inv_sigma")
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_ffa_create(self._ctx, self.num_series, self.p_lo, self.p_hi, self.log2_rows, self.num_widths,
                                       None if m is None else _hp(m), None if g is None else _hp(g), C.byref(self._h)), "mi355_ffa_create")

    @staticmethod
    def plan(num_series, p_lo, p_hi, log2_rows, num_widths):
        """(N = input floats per series, records per series, profile floats per series, scratch bytes of a handle); no device"""
        n, r, f, sb = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(lib().mi355_ffa_plan(int(num_series), int(p_lo), int(p_hi), int(log2_rows), int(num_widths), C.byref(n), C.byref(r), C.byref(f),
                                   C.byref(sb)), "mi355_ffa_plan")
        return n.value, r.value, f.value, sb.value

    def route(self):
        return self._L.mi355_ffa_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_ffa_set_generic(self._h, 1 if on else 0), "mi355_ffa_set_generic")

    def set_stats(self, mean, inv_sigma):
        check(self._L.mi355_ffa_set_stats(self._h, _hp(self._per_series(mean, "mean")), _hp(self._per_series(inv_sigma, "inv_sigma"))),
              "mi355_ffa_set_stats")

    def stats(self):
        m, g = np.empty(self.num_series, np.float32), np.empty(self.num_series, np.float32)
        check(self._L.mi355_ffa_get_stats(self._h, _hp(m), _hp(g), self.num_series), "mi355_ffa_get_stats")
        return m, g

    shift = staticmethod(ffa_shift)

    def period(self, p, i, tsamp_s=1.0):
        return ffa_period(p, self.log2_rows, i, tsamp_s)

    def in_floats(self, in_pitch=None):
        """floats from the first to one past the last a call reads"""
        return (self.num_series - 1) * (self.N if in_pitch is None else int(in_pitch)) + self.N

    def work(self, input_items, output_items, in_pitch=None):
        """host buffers: input_items[0] float32 x[s in_pitch + t]; output_items[0] an FFA_PEAK array of S x P x 2^L records;
        output_items[1], optional or None: the profiles, float32 S x P x 2^L x p_hi (the floats j >= p of a row keep their content)"""
        pitch = self.N if in_pitch is None else int(in_pitch)
        x = _host(input_items[0], np.float32)
        if pitch >= self.N:
            _need("input", x, self.in_floats(pitch))
        y = _host(output_items[0], FFA_PEAK, writable=True)
        _need("output", y, self.num_series * self.records)
        prof = None
        if len(output_items) > 1 and output_items[1] is not None:
            prof = _host(output_items[1], np.float32, writable=True)
            _need("output 1", prof, self.num_series * self.profile_floats)
        check(self._L.mi355_ffa_work(self._h, _hp(x), pitch, _hp(y), None if prof is None else _hp(prof)), "mi355_ffa_work")
        return 1

    def work_device(self, input_items, output_items, in_pitch=None):
        """CUDA tensors, enqueue only on torch's current stream; the same buffers as work(), 8 bytes per record (see peaks_of)"""
        pitch = self.N if in_pitch is None else int(in_pitch)
        xin = _dp(input_items[0], self.in_floats(pitch) * 4 if pitch >= self.N else None, "input")
        prof = None
        if len(output_items) > 1 and output_items[1] is not None:
            prof = _dp(output_items[1], 4 * self.num_series * self.profile_floats, "output 1")
        check(self._L.mi355_ffa_work_dev(self._h, xin, pitch, _dp(output_items[0], 8 * self.num_series * self.records, "output"), prof,
                                         _torch_stream(self.device)), "mi355_ffa_work_dev")
        return 1

    def search(self, x, in_pitch=None, profiles=False):
        """work() on a numpy input: the records as an FFA_PEAK array [S][P][2^L], or with profiles (records, float32 [S][P][2^L][p_hi],
        NaN where j >= p)"""
        y = np.empty((self.num_series, self.num_periods, self.num_rows), FFA_PEAK)
        if not profiles:
            self.work([x], [y], in_pitch)
            return y
        prof = np.full((self.num_series, self.num_periods, self.num_rows, self.p_hi), np.nan, np.float32)
        self.work([x], [y, prof], in_pitch)
        return y, prof

    def best(self, peaks):
        """(series, period in samples as a Fraction, k, j, snr) of the largest record of search()'s result: the greatest S/N, then the
        smallest k, then the smallest j, then the first in the array's order; None where no record holds a value"""
        from fractions import Fraction
        y = np.asarray(peaks).reshape(self.num_series, self.num_periods, self.num_rows)
        ok = y["loc"] != 0xFFFFFFFF
        if not ok.any():
            return None
        snr = np.where(ok, y["snr"], -np.inf)
        cand = np.flatnonzero((snr == snr.max()) & ok)
        at = cand[np.argmin(y["loc"].reshape(-1)[cand])]
        s, pi, i = np.unravel_index(at, y.shape)
        loc = int(y["loc"][s, pi, i])
        return int(s), self.p_lo + int(pi) + Fraction(int(i), max(self.num_rows - 1, 1)), loc >> 24, loc & 0xFFFFFF, float(y["snr"][s, pi, i])


SSEARCH_SERIES, SSEARCH_SPECTRUM = 0, 1
SSEARCH_PEAK, SSEARCH_CAND = PSEARCH_PEAK, PSEARCH_CAND


def ssearch_freq(n, tsamp_s, h, k):
    """the fundamental in Hz of bin k of harmonic-sum level h of clSpectralSearch (mi355_ssearch_freq, host only): k / (2^h n tsamp_s);
    its reciprocal is the period fold_model() takes"""
    v = lib().mi355_ssearch_freq(int(n), float(tsamp_s), int(h), int(k))
    if v != v:
        raise ValueError("ssearch_freq: an argument outside the block's ranges")
    return v


class clSpectralSearch(_PeakSearch):
    """FFT periodicity search with exact harmonic sums behind clDedisperser's per-trial output (beyond the reference module; the
    contract is in include/mi355_clenabled.h).  SERIES input: every series of n samples is transformed (an internal clFFT of n / 2
    points, untangled) into the normalised power spectrum w[k] = |X[k]|^2 inv_sigma^2 / n, k < n / 2, +0 below k_lo -- floating point,
    held to a derived bound.  Then, bit-exact: level h <= num_folds adds the 2^h - 1 lower harmonics w[(k j + 2^(h-1)) >> h] to w[k] in
    a pinned order, snr_h[k] = (s_h[k] - 2^h) c_h, and every (series, block of block_bins bins) gives the record {snr, loc = (h << 24) |
    k_in_block} of its largest value (ties: smallest h, then smallest k; NaN never takes part): peaks[s][b].  SPECTRUM input runs the
    sums on a given w.  With max_cands > 0 every peak at or above the threshold is also listed: candidates()."""
    _destroy = "mi355_ssearch_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, num_series, n, num_folds, block_bins, k_lo=1,
                 input_kind=SSEARCH_SERIES, inv_sigma=None, max_cands=0, setDebug=0):
        self.num_series, self.n, self.num_folds, self.block_bins = int(num_series), int(n), int(num_folds), int(block_bins)
        self.k_lo, self.input_kind, self.max_cands = int(k_lo), int(input_kind), int(max_cands)
        # argument errors before a context exists
        self.num_bins, self.records, self.scratch_bytes = self.plan(self.num_series, self.n, self.num_folds, self.block_bins, self.k_lo,
                                                                    self.input_kind)
        if self.max_cands < 0:
            raise ValueError("max_cands is negative")
        self.row = self.n if self.input_kind == SSEARCH_SERIES else self.num_bins  # floats of a series of the input
        g = None if inv_sigma is None else self._per_series(inv_sigma)
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_ssearch_create(self._ctx, self.num_series, self.n, self.num_folds, self.block_bins, self.k_lo, self.input_kind,
                                           None if g is None else _hp(g), C.byref(self._h)), "mi355_ssearch_create")

    @staticmethod
    def plan(num_series, n, num_folds, block_bins, k_lo=1, input_kind=SSEARCH_SERIES):
        """(spectrum floats per series = n / 2, records per series, scratch bytes of a handle); no device"""
        a, r, sb = C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(lib().mi355_ssearch_plan(int(num_series), int(n), int(num_folds), int(block_bins), int(k_lo), int(input_kind), C.byref(a),
                                       C.byref(r), C.byref(sb)), "mi355_ssearch_plan")
        return a.value, r.value, sb.value

    def route(self):
        return self._L.mi355_ssearch_route(self._h).decode()

    def fft_route(self):
        """clFFT.last_route() of the internal transform's last call ('' with SPECTRUM input or before the first call)"""
        return self._L.mi355_ssearch_fft_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_ssearch_set_generic(self._h, 1 if on else 0), "mi355_ssearch_set_generic")

    def set_threshold(self, threshold):
        check(self._L.mi355_ssearch_set_threshold(self._h, float(threshold)), "mi355_ssearch_set_threshold")

    def set_stats(self, inv_sigma):
        check(self._L.mi355_ssearch_set_stats(self._h, _hp(self._per_series(inv_sigma))), "mi355_ssearch_set_stats")

    def stats(self):
        g = np.empty(self.num_series, np.float32)
        check(self._L.mi355_ssearch_get_stats(self._h, _hp(g), self.num_series), "mi355_ssearch_get_stats")
        return g

    def freq(self, h, k, tsamp_s=1.0):
        return ssearch_freq(self.n, tsamp_s, h, k)

    def in_floats(self, in_pitch=None):
        """floats from the first to one past the last a call reads"""
        return (self.num_series - 1) * (self.row if in_pitch is None else int(in_pitch)) + self.row

    def work(self, input_items, output_items, in_pitch=None):
        """host buffers: input_items[0] float32, x[s in_pitch + t] (SERIES) or w[s in_pitch + k] (SPECTRUM); output_items[0] an
        SSEARCH_PEAK array of S x (n / 2 / block_bins) records; output_items[1], optional or None: the spectrum, float32 S x n / 2"""
        pitch = self.row if in_pitch is None else int(in_pitch)
        x = _host(input_items[0], np.float32)
        if pitch >= self.row:
            _need("input", x, self.in_floats(pitch))
        y = _host(output_items[0], SSEARCH_PEAK, writable=True)
        _need("output", y, self.num_series * self.records)
        spec = None
        if len(output_items) > 1 and output_items[1] is not None:
            spec = _host(output_items[1], np.float32, writable=True)
            _need("output 1", spec, self.num_series * self.num_bins)
        cands, counts = self._new_cands()
        check(self._L.mi355_ssearch_work(self._h, _hp(x), pitch, _hp(y), None if spec is None else _hp(spec),
                                         None if cands is None else _hp(cands), self.max_cands, None if counts is None else _hp(counts)),
              "mi355_ssearch_work")
        self._cands, self._counts = cands, counts
        return 1

    def work_device(self, input_items, output_items, in_pitch=None, cands=None, counts=None):
        """CUDA tensors, enqueue only on torch's current stream; the same buffers as work(), 8 bytes per record (see peaks_of).  cands
        and counts, if given, are the candidate buffer (16 max_cands bytes) and the two 32-bit counters, otherwise the block keeps its own"""
        pitch = self.row if in_pitch is None else int(in_pitch)
        xin = _dp(input_items[0], self.in_floats(pitch) * 4 if pitch >= self.row else None, "input")
        spec = None
        if len(output_items) > 1 and output_items[1] is not None:
            spec = _dp(output_items[1], 4 * self.num_series * self.num_bins, "output 1")
        if not self.max_cands or cands is None:
            cands, counts = self._new_cands(input_items[0])
        check(self._L.mi355_ssearch_work_dev(self._h, xin, pitch, _dp(output_items[0], 8 * self.num_series * self.records, "output"), spec,
                                             None if cands is None else _dp(cands, self.max_cands * 16, "candidates"), self.max_cands,
                                             None if counts is None else _dp(counts, 8, "counts"), _torch_stream(self.device)),
              "mi355_ssearch_work_dev")
        self._cands, self._counts = cands, counts
        return 1

    def search(self, x, in_pitch=None, spectrum=False):
        """work() on a numpy input: the records as an SSEARCH_PEAK array [S][n / 2 / block_bins], or with spectrum=True (records, w
        float32 [S][n / 2])"""
        y = np.empty((self.num_series, self.records), SSEARCH_PEAK)
        if not spectrum:
            self.work([x], [y], in_pitch)
            return y
        w = np.empty((self.num_series, self.num_bins), np.float32)
        self.work([x], [y, w], in_pitch)
        return y, w

    def best(self, peaks):
        """(series, h, k, snr) of the largest record of search()'s result, k the bin in the spectrum: the greatest S/N, then the smallest
        h, then the smallest k, then the first in the array's order; None where no record holds a value.  The fundamental is
        freq(h, k, tsamp_s)"""
        y = np.asarray(peaks).reshape(self.num_series, self.records)
        ok = y["loc"] != 0xFFFFFFFF
        if not ok.any():
            return None
        snr = np.where(ok, y["snr"], -np.inf)
        full = (y["loc"] & np.uint32(0xFF000000)).astype(np.uint64) << np.uint64(8) | (
            np.arange(self.records, dtype=np.uint64)[None, :] * np.uint64(self.block_bins) + (y["loc"] & np.uint32(0xFFFFFF)))
        cand = np.flatnonzero((snr == snr.max()) & ok)
        at = cand[np.argmin(full.reshape(-1)[cand])]
        s, b = np.unravel_index(at, y.shape)
        loc = int(y["loc"][s, b])
        return int(s), loc >> 24, int(b) * self.block_bins + (loc & 0xFFFFFF), float(y["snr"][s, b])


ACCEL_LIGHT_M_S = 299792458.0


def accel_coeff(n, tsamp_s, accel_m_s2):
    """the coefficient c of clAccelResampler's index map for a line-of-sight acceleration in m/s^2 (mi355_accel_coeff, host only, computed
    in long double): round(-2^64 accel tsamp / (2 x 299792458)), a Python int"""
    c = C.c_longlong()
    check(lib().mi355_accel_coeff(int(n), float(tsamp_s), float(accel_m_s2), C.byref(c)), "mi355_accel_coeff")
    return c.value


def accel_index(n, c, i0=0, count=None):
    """src(i) of i = i0 .. i0 + count - 1 (to the end of the series by default) for one coefficient, bit for bit as clAccelResampler
    computes it (mi355_accel_index, host only): int64 [count]"""
    count = int(n) - int(i0) if count is None else int(count)
    out = np.empty(max(count, 0), np.int64)
    check(lib().mi355_accel_index(int(n), int(c), int(i0), count, _hp(out)), "mi355_accel_index")
    return out


def accel_trials(n, tsamp_s, a_lo, a_hi, tol_samples=1.0, cap=None):
    """the ladder of coefficients whose neighbours differ by tol_samples samples at mid-observation, accelerations j da inside
    [a_lo, a_hi] (mi355_accel_trials, host only): (int64 [min(count, cap)], count); cap None stores the whole ladder"""
    cnt = C.c_longlong()
    if cap is None:
        check(lib().mi355_accel_trials(int(n), float(tsamp_s), float(a_lo), float(a_hi), float(tol_samples), None, 0, C.byref(cnt)),
              "mi355_accel_trials")
        cap = cnt.value
    out = np.zeros(int(cap), np.int64)
    check(lib().mi355_accel_trials(int(n), float(tsamp_s), float(a_lo), float(a_hi), float(tol_samples), _hp(out), int(cap), C.byref(cnt)),
          "mi355_accel_trials")
    return out[:min(int(cap), cnt.value)], cnt.value


class clAccelResampler(_Block):
    """Exact acceleration trials behind clDedisperser's per-trial output (beyond the reference module; the contract is in
    include/mi355_clenabled.h).  Every series of n 32-bit words is stretched quadratically once per trial a, with the integer index
    src_a(i) = i + floor((c[a] i (n - i) + 2^63) / 2^64): out[(s na + (a - a0)) out_pitch + i] = in[s in_pitch + src_a(i)].  The
    words are moved, never computed on; the num_series x na output rows are series for clSpectralSearch, clPeriodSearch and
    clPulseSearch.measure() as they lie.  `trials`: num_trials signed 64-bit coefficients (accel_coeff(), accel_trials())."""
    _destroy = "mi355_accel_destroy"

    def __init__(self, openCLPlatformType, devSelector, platformId, devId, num_series, n, trials, setDebug=0):
        self.num_series, self.n = int(num_series), int(n)
        t = self._table(trials, None)
        self.num_trials = int(t.size)
        # argument errors before a context exists
        self.rows, self.tile, self.table_bytes = self.plan(self.num_series, self.n, self.num_trials)
        super().__init__(openCLPlatformType, devSelector, platformId, devId, setDebug)
        check(self._L.mi355_accel_create(self._ctx, self.num_series, self.n, self.num_trials, _hp(t), C.byref(self._h)), "mi355_accel_create")

    @staticmethod
    def plan(num_series, n, num_trials):
        """(output rows of the whole ladder = num_series x num_trials, outputs per tile, bytes of the device table); no device"""
        r, t, b = C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(lib().mi355_accel_plan(int(num_series), int(n), int(num_trials), C.byref(r), C.byref(t), C.byref(b)), "mi355_accel_plan")
        return r.value, t.value, b.value

    @staticmethod
    def _table(trials, size):
        t = np.ascontiguousarray(trials).reshape(-1)
        if t.dtype != np.int64:
            if t.dtype.kind not in "iu" and t.dtype != object:
                raise TypeError("trials are signed 64-bit integers")
            t = np.array([int(v) for v in t], np.int64)  # OverflowError for a value that is no int64
        if size is not None and t.size != size:
            raise ValueError("trials hold %d entries, the block has %d trials" % (t.size, size))
        return t

    def route(self):
        return self._L.mi355_accel_route(self._h).decode()

    def set_generic(self, on):
        check(self._L.mi355_accel_set_generic(self._h, 1 if on else 0), "mi355_accel_set_generic")

    def set_trials(self, trials):
        check(self._L.mi355_accel_set_trials(self._h, _hp(self._table(trials, self.num_trials))), "mi355_accel_set_trials")

    def trials(self):
        c = np.empty(self.num_trials, np.int64)
        check(self._L.mi355_accel_get_trials(self._h, _hp(c), self.num_trials), "mi355_accel_get_trials")
        return c

    def _range(self, a0, na):
        a0 = int(a0)
        return a0, self.num_trials - a0 if na is None else int(na)

    def in_words(self, in_pitch=None):
        """words from the first to one past the last a call reads"""
        return (self.num_series - 1) * (self.n if in_pitch is None else int(in_pitch)) + self.n

    def out_words(self, na, out_pitch=None):
        """words from the first to one past the last a call of na trials writes"""
        return (self.num_series * int(na) - 1) * (self.n if out_pitch is None else int(out_pitch)) + self.n

    def series_to_trial(self, row, a0=0, na=None):
        """(series, trial) of output row `row` of a call over the trial range [a0, a0 + na)"""
        a0, na = self._range(a0, na)
        if not 0 <= int(row) < self.num_series * na:
            raise ValueError("row %d is outside the %d rows of the call" % (row, self.num_series * na))
        return int(row) // na, a0 + int(row) % na

    def work(self, input_items, output_items, a0=0, na=None, in_pitch=None, out_pitch=None):
        """host buffers of 4-byte items (float32, int32 or uint32): input_items[0] x[s in_pitch + i]; output_items[0]
        y[(s na + (a - a0)) out_pitch + i]"""
        a0, na = self._range(a0, na)
        ip, op = self.n if in_pitch is None else int(in_pitch), self.n if out_pitch is None else int(out_pitch)
        x, y = _host(input_items[0]), _host(output_items[0], writable=True)
        if x.dtype.itemsize != 4 or y.dtype.itemsize != 4:
            raise TypeError("clAccelResampler moves 4-byte items")
        if ip >= self.n:
            _need("input", x, self.in_words(ip))
        if op >= self.n and 1 <= na <= self.num_trials:
            _need("output", y, self.out_words(na, op))
        check(self._L.mi355_accel_work(self._h, _hp(x), ip, _hp(y), op, a0, na), "mi355_accel_work")
        return 1

    def work_device(self, input_items, output_items, a0=0, na=None, in_pitch=None, out_pitch=None):
        """CUDA tensors of 4-byte items, enqueue only on torch's current stream; the same buffers as work()"""
        a0, na = self._range(a0, na)
        ip, op = self.n if in_pitch is None else int(in_pitch), self.n if out_pitch is None else int(out_pitch)
        xin = _dp(input_items[0], self.in_words(ip) * 4 if ip >= self.n else None, "input")
        yout = _dp(output_items[0], self.out_words(na, op) * 4 if op >= self.n and 1 <= na <= self.num_trials else None, "output")
        check(self._L.mi355_accel_work_dev(self._h, xin, ip, yout, op, a0, na, _torch_stream(self.device)), "mi355_accel_work_dev")
        return 1

    def resample(self, x, a0=0, na=None, in_pitch=None):
        """work() on a numpy input: the output [num_series][na][n] of the input's dtype"""
        a0, na = self._range(a0, na)
        x = _host(x)
        y = np.empty((self.num_series, na, self.n), x.dtype)
        self.work([x], [y], a0, na, in_pitch)
        return y
