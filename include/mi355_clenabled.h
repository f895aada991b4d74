/*
 * mi355_clenabled.h -- C ABI of the MI355X (gfx950) streaming-DSP hot path that
 * replaces gr-clenabled's OpenCL runtime shim and kernel bodies.
 *
 * This is the drop-in boundary: the reference's block implementations
 * (lib/cl*_impl.cc) inherit GRCLBase (include/clenabled/GRCLBase.h:77-141,
 * lib/GRCLBase.cpp:17-474) and call cl::CommandQueue / clFFT from work();
 * a gr-clenabled maintainer binds the entry points below instead (see
 * INTEGRATION.md for the exact _impl stubs).  Plain C, opaque handles, raw
 * pointers and sizes only; nothing here throws or calls exit().
 *
 * Conventions
 *   - every function returns MI355_OK (0) or a negative MI355_ERR_* code;
 *     mi355_last_error() gives the thread's last diagnostic string;
 *   - gr_complex == { float re, im } interleaved, 8 bytes
 *     (include/clenabled/clSComplex.h:12-17);
 *   - `*_work(...)`     take HOST pointers, exactly what GNU Radio hands a
 *     block's work(); the call stages through pinned double buffers
 *     (H2D / kernel / D2H overlapped on two HIP streams) and returns when the
 *     output is complete -- the contract of the reference's blocking
 *     enqueueReadBuffer (e.g. lib/clMathOp_impl.cc:438);
 *   - `*_work_dev(...)` take DEVICE pointers plus a hipStream_t (as void*; NULL
 *     = HIP's default stream; pass mi355_ctx_stream() for the context's own)
 *     and only enqueue: this is the device-resident path chained blocks and
 *     the benchmarks use;
 *   - there is NO CPU fallback: OCLTYPE_CPU (3) is refused with
 *     MI355_ERR_UNSUPPORTED and every call fails loudly without a gfx950 GPU.
 */
#ifndef MI355_CLENABLED_H
#define MI355_CLENABLED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK               0
#define MI355_ERR_INVALID_ARG (-1)
#define MI355_ERR_NO_DEVICE   (-2)
#define MI355_ERR_UNSUPPORTED (-3)
#define MI355_ERR_HIP         (-4)
#define MI355_ERR_NOMEM       (-5)
#define MI355_ERR_STATE       (-6)

/* data types: include/clenabled/GRCLBase.h:57-62 */
#define MI355_DTYPE_COMPLEX  1
#define MI355_DTYPE_FLOAT    2
#define MI355_DTYPE_INT      3
#define MI355_DTYPE_SHORT    4
#define MI355_DTYPE_BYTE     5
#define MI355_DTYPE_PACKEDXY 6
/* device selection: include/clenabled/GRCLBase.h:64-70 */
#define MI355_OCLTYPE_GPU         1
#define MI355_OCLTYPE_ACCELERATOR 2
#define MI355_OCLTYPE_CPU         3
#define MI355_OCLTYPE_ANY         4
#define MI355_DEVSEL_FIRST    1
#define MI355_DEVSEL_SPECIFIC 2
/* operators: include/clenabled/clMathOpTypes.h:11-20 */
#define MI355_OP_MULTIPLY           1
#define MI355_OP_ADD                2
#define MI355_OP_SUBTRACT           3
#define MI355_OP_COMPLEX_CONJUGATE  4
#define MI355_OP_MULTIPLY_CONJUGATE 5
#define MI355_OP_EMPTY_W_COPY     254
#define MI355_OP_EMPTY            255
/* FFT direction as GRC passes it (clFFT's enum; lib/clFFT_impl.cc:84-89,
 * grc/clenabled_clFFT.block.yml:37-41) */
#define MI355_FFT_FORWARD  (-1)
#define MI355_FFT_BACKWARD   1

typedef struct mi355_ctx     mi355_ctx;
typedef struct mi355_mathop  mi355_mathop;
typedef struct mi355_mathconst mi355_mathconst;
typedef struct mi355_fft     mi355_fft;
typedef struct mi355_filter  mi355_filter;
typedef struct mi355_pfb     mi355_pfb;
typedef struct mi355_xengine mi355_xengine;
typedef struct mi355_elem    mi355_elem;
typedef struct mi355_xcorr_fft mi355_xcorr_fft;
typedef struct mi355_xcorr_td mi355_xcorr_td;
typedef struct mi355_sigsource mi355_sigsource;
typedef struct mi355_costas  mi355_costas;

/* ---------------------------------------------------------------------------
 * Runtime: replaces GRCLBase::InitOpenCL / cleanup (lib/GRCLBase.cpp:17-369,
 * 423-474) and the ctor arguments (include/clenabled/GRCLBase.h:136-137).
 * ------------------------------------------------------------------------- */
const char *mi355_strerror(int code);
const char *mi355_last_error(void);
const char *mi355_version(void);
/* Diagnostics sink.  The reference writes through GNU Radio's logger (GR_LOG_INFO / GR_LOG_ERROR, lib/clXEngine_impl.cc:107,
 * 137,257) and to std::cout when setDebug is on (lib/GRCLBase.cpp:96-120); a C library has neither, so the block layer hands
 * its logger in here.  Process wide; fn == NULL restores the default (DEBUG/INFO lines of a context created with debug != 0 go
 * to stderr, errors are only kept for mi355_last_error()).  The callback receives every such line and every error message at
 * MI355_LOG_ERROR, on the calling thread, with no lock held; `message` is valid only during the call. */
#define MI355_LOG_DEBUG 0
#define MI355_LOG_INFO  1
#define MI355_LOG_WARN  2
#define MI355_LOG_ERROR 3
typedef void (*mi355_log_fn)(void *user, int level, const char *message);
int mi355_set_log_callback(mi355_log_fn fn, void *user);
/* number of gfx950 devices visible, or a negative error */
int mi355_device_count(void);
/* ocl_type 1/2/4 -> HIP device; 3 (CPU) -> MI355_ERR_UNSUPPORTED.
 * dev_selector FIRST -> ordinal 0; SPECIFIC -> ordinal dev_id (platform_id must
 * be 0: there is one HIP platform). */
int mi355_ctx_create(int ocl_type, int dev_selector, int platform_id, int dev_id, int debug, mi355_ctx **out);
int mi355_ctx_destroy(mi355_ctx *ctx);
int mi355_ctx_device(const mi355_ctx *ctx);
/* the context's compute stream (hipStream_t) */
void *mi355_ctx_stream(mi355_ctx *ctx);
int mi355_ctx_synchronize(mi355_ctx *ctx);
/* device memory helpers for callers without their own allocator (C++ harness) */
int mi355_malloc(mi355_ctx *ctx, size_t bytes, void **dptr);
int mi355_free(mi355_ctx *ctx, void *dptr);
int mi355_memcpy_h2d(mi355_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int mi355_memcpy_d2h(mi355_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* Device-side strided block copy, dst[b][r][0..width) = src[b][r][0..width) for b < nblocks, r < rows, with independent
 * row pitches and block strides (bytes).  Used to pack the per-peer channel slices of the X-engine's all-to-all corner
 * turn (the reference has no multi-device path). */
int mi355_pack3d_dev(mi355_ctx *ctx, void *dst_dev, const void *src_dev, size_t width_bytes, size_t rows, size_t nblocks,
                     size_t src_pitch, size_t src_block_stride, size_t dst_pitch, size_t dst_block_stride, void *stream);

/* ---------------------------------------------------------------------------
 * clMathOp: c = a (op) b.  Replaces clMathOp_impl::processOpenCL
 * (lib/clMathOp_impl.cc:361-442) and its kernels (:104-238).
 * dtype COMPLEX/FLOAT/INT; op MULTIPLY/ADD/SUBTRACT (+MULTIPLY_CONJUGATE for
 * complex).  max_items is a sizing hint (0 -> 8192, :80-84); buffers grow.
 * ------------------------------------------------------------------------- */
int mi355_mathop_create(mi355_ctx *ctx, int dtype, int op, size_t max_items, mi355_mathop **out);
int mi355_mathop_destroy(mi355_mathop *h);
int mi355_mathop_work(mi355_mathop *h, size_t nitems, const void *a, const void *b, void *c);
int mi355_mathop_work_dev(mi355_mathop *h, size_t nitems, const void *a, const void *b, void *c, void *stream);

/* ---------------------------------------------------------------------------
 * clMathConst: c = a (op) k with a REAL scalar k applied to both components of
 * a complex item.  Replaces clMathConst_impl::processOpenCL
 * (lib/clMathConst_impl.cc:311-361), kernels (:100-225), k()/set_k()
 * (lib/clMathConst_impl.h:107-108).  op MULTIPLY/ADD/SUBTRACT,
 * COMPLEX_CONJUGATE (complex only), EMPTY_W_COPY (copy), EMPTY (no-op launch).
 * ------------------------------------------------------------------------- */
int mi355_mathconst_create(mi355_ctx *ctx, int dtype, int op, float k, size_t max_items, mi355_mathconst **out);
int mi355_mathconst_destroy(mi355_mathconst *h);
int mi355_mathconst_set_k(mi355_mathconst *h, float k);
int mi355_mathconst_get_k(const mi355_mathconst *h, float *k);
int mi355_mathconst_work(mi355_mathconst *h, size_t nitems, const void *a, void *c);
int mi355_mathconst_work_dev(mi355_mathconst *h, size_t nitems, const void *a, void *c, void *stream);

/* ---------------------------------------------------------------------------
 * clFFT: per frame Y = [fftshift] FFT_N( x .* window ), unnormalised in both
 * directions.  Replaces the clFFT plan + MultiplyFloat kernel + host fftshift
 * of clFFT_impl (ctor lib/clFFT_impl.cc:65-151, processOpenCL :526-634).
 * fft_size: any power of two 2..32768 (one fused kernel), 65536..1048576 (two passes over 16-column tiles), 2097152..16777216
 * (four passes; 2^24 is clFFT's own single-precision limit); lengths 2^a 3^b 5^c 7^d 11^e 13^f up to 15360 (14336 / 13312 / 11264 with a factor 7 / 13 / 11) that are not a power of two in
 * one pass by a mixed-radix kernel (the lengths clFFT's radix-3/5/7 plans cover; its workgroup shape is measured once per length
 * and process at create, about 20 ms), such lengths up to 921600 (= N1 x N2, both at most 960) in two passes; any other size 3..8388608 by chirp-z over the power-of-two kernels (the reference
 * leaves those to clFFT, which refuses prime factors above 13);
 * larger sizes return MI355_ERR_UNSUPPORTED.  The shift of an odd-sized frame follows
 * clFFT_impl::testCPU (len = ceil(N/2), :503-507).  window: NULL/0 or exactly fft_size floats
 * (:74-76).  dtype COMPLEX or FLOAT (real input, complex output).
 * `nvec` = number of frames per stream (= noutput_items of work(), :637-654).
 * ------------------------------------------------------------------------- */
int mi355_fft_create(mi355_ctx *ctx, int fft_size, int direction, const float *window, int window_len,
                     int dtype, int num_streams, int shift, mi355_fft **out);
int mi355_fft_destroy(mi355_fft *h);
/* Which path a length takes, as text ("one pass", "two tile passes 256 x 512", "mixed radix 10 x 10 x 10",
 * "chirp-z, m = 8192 (fused)", ...): planning only, no device is touched.  Returns MI355_OK, or MI355_ERR_UNSUPPORTED with the
 * reason in buf for a length mi355_fft_create would refuse. */
int mi355_fft_plan_text(int fft_size, char *buf, int buf_len);
int mi355_fft_work(mi355_fft *h, int nvec, const void *const *in_streams, void *const *out_streams);
/* Concurrency: sizes up to 32768 are stateless (any number of work_dev calls of one handle may be in flight on any streams).
 * 65536 points and more, and the non-power-of-two sizes above 2048, go through ONE per-handle workspace: calls from different threads or
 * streams are accepted and serialised on it (the later stream waits for the earlier call's kernels); use one handle per
 * stream for overlap.  Sizes: powers of two 2 .. 16777216, any other length 3 .. 8388608 (chirp-z); larger ones return
 * MI355_ERR_UNSUPPORTED. */
int mi355_fft_work_dev(mi355_fft *h, int nvec, const void *in, void *out, void *stream);
/* The kernels the last work / work_dev of this handle launched and the parameters that change the arithmetic or the schedule:
 * "k_fft<64> PF=0", "k_fft<4096> PF=1 dyn grid=512" (persistent loop with the next group in flight; dyn / static: frame groups by claims
 * or by the grid stride), "k_fft_s<8192>", "k_fft_32k", "k_fft_tile 256x512", "k_fft_sub+combine2 S=16x16x2" (2^21 points and more; the
 * last factor is the radix of the last combine), "k_fft_mr 10x10x10 threads=256 frames=3", "k_fft_mr_tile 100 x 160 (10x10, 10x16)" (two passes and the radices inside either), "k_chirpz<8192>",
 * "bluestein m=65536: k_fft_tile 256x256" (the unfused chirp-z path and the route of its size-m transforms).  "" before the first
 * call.  Valid until the handle's next call; recorded without a lock, so with two streams on one handle it is either call's. */
const char *mi355_fft_last_route(mi355_fft *h);
/* Which input items an output depends on.  Output frame f (items [f N, (f + 1) N) of out) depends on input frame f alone, on every route
 * and schedule, however many frames a workgroup holds and whichever workgroup picks the frame up.  A non-finite item in frame f
 * makes every bin of frame f non-finite -- complex input with both components non-finite: both components of every bin; real
 * input: at least one component of every bin (a bin whose twiddle is 1 or -1 keeps the imaginary part 0 + 0) -- and every other frame
 * has the bits of the same call without it.  A frame of zeros comes out as zeros. */

/* ---------------------------------------------------------------------------
 * clFilter / clComplexFilter: decimating FIR on a complex stream,
 *     y[m] = sum_k h[k] * x[m*decimation - k]
 * Replaces clFilter_impl (ctor lib/clFilter_impl.cc:50-83, filterGPUTimeDomain
 * :504-589, filterGPUFrequencyDomain :591-681, set_taps2 :441-479) and
 * clComplexFilter_impl::filterGPU (lib/clComplexFilter_impl.cc:959-1030).
 * `in` is GNU Radio's history-prefixed buffer (set_history(ntaps), :78):
 * in[ntaps-1] is x[0]; noutput*decimation + ntaps - 1 samples are read.
 * use_time = 0 : fused overlap-save fast convolution (FFT -> xH -> IFFT in LDS); the transform size is chosen
 *                for throughput (>= the reference's 2*2^ceil(log2 ntaps), lib/fft_filter.cc:72-97); a filter longer
 *                than 2048 taps is partitioned into ceil(ntaps/2048) segments whose spectra are applied to delayed
 *                input blocks and summed before ONE inverse transform per block (same y; 10-25x the direct form's rate)
 * use_time = 1 : direct-form tap dot product
 * complex_taps = 1 : taps is ntaps gr_complex (clComplexFilter), else floats.
 * ------------------------------------------------------------------------- */
int mi355_filter_create(mi355_ctx *ctx, int decimation, const void *taps, int ntaps, int complex_taps,
                        int use_time, mi355_filter **out);
int mi355_filter_destroy(mi355_filter *h);
/* takes effect at the next call; calls already enqueued keep what they were given */
int mi355_filter_set_taps(mi355_filter *h, const void *taps, int ntaps);
int mi355_filter_ntaps(const mi355_filter *h);
int mi355_filter_get_taps(const mi355_filter *h, void *taps_out, int cap);
/* FFT size the fast-convolution kernel runs (0 in time-domain mode; 4096 for partitioned filters of more than 2048 taps) */
int mi355_filter_fftsize(const mi355_filter *h);
int mi355_filter_work(mi355_filter *h, size_t noutput_items, const void *in_with_history, void *out);
int mi355_filter_work_dev(mi355_filter *h, size_t noutput_items, const void *in_with_history, void *out, void *stream);
/* The kernel the last work / work_dev of this handle launched and the parameters that matter, e.g. "k_fir_td<real>", "k_fir_mfma<complex,dec>",
 * "k_fir_dec2<real,odd> tile_out=166", "k_fir_dec_lds<real> tile_out=32", "k_fir_td_dec<real>", "k_ols<256>"; "" before the first call.  Valid
 * until the handle's next call. */
const char *mi355_filter_last_route(mi355_filter *h);
/* Which input items an output depends on (direct form, use_time = 1).  Output m reads items [m D, m D + K) of the history-prefixed input
 * (D = decimation, K = ntaps).  A non-finite item s makes every output whose window holds s non-finite.  The kernels pad the taps with
 * zeros that multiply neighbouring samples (0 x NaN = NaN), so s may also make non-finite outputs with m D - PAD <= s < m D + K + PAD and
 * no others: every other output has the bits of the same call without it.  PAD = 18 items, the largest over the kernels: k_fir_mfma
 * multiplies blocks of 16 undecimated outputs by K + 15 samples rounded up to a multiple of four (15 items before a window, 18 behind);
 * k_fir_td and k_fir_dec2 round K up to a multiple of 8 (7 items behind); k_fir_dec_lds and k_fir_td_dec read the window alone.
 * The fast-convolution mode (use_time = 0) spreads a non-finite item over every output of the transform blocks that hold it. */

/* ---------------------------------------------------------------------------
 * clPolyphaseChannelizer: M-branch polyphase filterbank + M-point backward DFT
 * + channel map, one multiplexed output stream.  Replaces
 * clPolyphaseChannelizer_impl (ctor lib/clPolyphaseChannelizer_impl.cc:47-67,
 * general_work :83-109, kernels :153-177, clFFT plan :208-225).
 * One call consumes buf_items inputs and produces nmap*buf_items/ninputs_per_iter
 * outputs.  `in` is history-prefixed (set_history(ntaps), :63) and must hold
 * buf_items - ninputs_per_iter + ntaps samples.
 * ------------------------------------------------------------------------- */
int mi355_pfb_create(mi355_ctx *ctx, const float *taps, int ntaps, int buf_items, int num_channels,
                     int ninputs_per_iter, const int *ch_map, int nmap, mi355_pfb **out);
int mi355_pfb_destroy(mi355_pfb *h);
int mi355_pfb_noutput(const mi355_pfb *h);
int mi355_pfb_ninput(const mi355_pfb *h);
int mi355_pfb_work(mi355_pfb *h, const void *in_with_history, void *out);
int mi355_pfb_work_dev(mi355_pfb *h, const void *in_with_history, void *out, void *stream);
/* nbuf consecutive buffers in one launch (general_work() offered nbuf output multiples): in holds
 * nbuf * buf_items - ninputs_per_iter + ntaps samples, out nbuf * noutput().  Same samples as nbuf single calls. */
int mi355_pfb_work_dev_n(mi355_pfb *h, int nbuf, const void *in_dev, void *out_dev, void *stream);
/* The kernels the last call of this handle launched, e.g. "k_pfbw<64,32>", "k_pfbq<256,8>", "k_pfbs<32,8>", "k_pfb<8,16>" (staged),
 * "k_pfbw<64,8,over=2>", "k_pfb_mr<16>", "k_pfb_fir<32> + clFFT", "k_pfb_branches_t<8,16,1> + clFFT + k_pfb_map",
 * "k_pfb_branches + k_pfb_dft_map"; "" before the first call.  Valid until the handle's next call. */
const char *mi355_pfb_last_route(mi355_pfb *h);
/* Which input items a step depends on.  Step i (R = ninputs_per_iter, M = num_channels, K = ntaps) reads items [i R, i R + K) of the
 * history-prefixed input, item s with tap k = i R + K - 1 - s; every mapped channel of a step depends on all of them (the M-point DFT).
 * A non-finite item s makes every mapped channel of the steps ceil((s - K + 1) / R) ... floor(s / R) non-finite.  For R = M, with s in
 * input row r = ceil((s - K + 1) / M) and P the taps of its arm, these are the steps r ... r + P - 1.  The kernels round the taps per arm
 * up with zeros (0 x NaN = NaN), so s may also reach the steps up to floor((s - K + PMAXR M) / R) -- for R = M the steps up to
 * r + PMAXR - 1, for R < M as many more steps as fit PMAXR rows of M items -- never a step before the first one named and never a later
 * one; every other step has the bits of the same call without it.  PMAXR = 32 steps for up to 32 taps per arm, the largest over the
 * kernels: the fused kernels (k_pfbs, k_pfbq, k_pfbw, k_pfb, k_pfb_mr) round the taps per arm up to 8, 16 or 32, k_pfb_fir to 8 or 32,
 * k_pfb_branches_t to a multiple of 16 (8 and 4 when 2- and 4-fold oversampled), k_pfb_branches reads the window alone.  Longer arms: the
 * fused power-of-two kernels round 33 ... 64 taps per arm up to 64, k_pfb_branches_t rounds up to its multiple (at most 15 more). */

/* ---------------------------------------------------------------------------
 * clXEngine: V[f][k][pol2] = sum_t x_s1(t,f) conj(x_s2(t,f)), k = s1(s1+1)/2+s2.
 * Replaces clXEngine_impl's device side: xcorrelate() overloads
 * (lib/clXEngine_impl.h:150-201), kernels (lib/clXEngine_impl.cc:605-916),
 * accumulator zero/"+=" for pipeline integration (:289-292,785-796), and the
 * host frame gather of work_processor (:987-1061).
 * data_type COMPLEX (cf32), BYTE (int8 I,Q) or PACKEDXY (4-bit, npol forced 2).
 * Input layout [t][station][chan][pol]; output matrix_flat_length =
 * nchan * ninputs(ninputs+1)/2 * npol^2 gr_complex, triangular order.
 * ------------------------------------------------------------------------- */
int mi355_xengine_create(mi355_ctx *ctx, int data_type, int npol, int num_inputs, int num_channels,
                         int integration, mi355_xengine **out);
int mi355_xengine_destroy(mi355_xengine *h);
size_t mi355_xengine_input_bytes(const mi355_xengine *h);
size_t mi355_xengine_output_items(const mi355_xengine *h);
/* accumulate=0: out = V ; accumulate=1: out += V (pipeline integration) */
int mi355_xengine_xcorrelate(mi355_xengine *h, const void *in_host, void *out_host, int accumulate);
/* (device-pointer calls: a handle may be used from several streams -- launches that share the handle's partial-sum workspace are ordered by the
 * library when the stream changes: behind one of the context's own streams with an event, behind a caller's stream -- which may have been
 * destroyed since, and is therefore never touched again -- by waiting for the device.  A stream may be destroyed as soon as the caller is done
 * with it.  Batched launches that need no workspace -- no time ranges -- are not ordered at all.) */
int mi355_xengine_xcorrelate_dev(mi355_xengine *h, const void *in_dev, void *out_dev, int accumulate, void *stream);
/* Multi-GPU form (no counterpart in the reference, which runs one X-engine on one device): the input is the
 * receive buffer of the all-to-all corner turn, [group][t][station in group][chan][pol], stations_per_group stations per
 * sending rank; it is read in place.  IChar geometries of the fused path only (<= 64 rows, rows of whole 16-byte pieces),
 * otherwise MI355_ERR_UNSUPPORTED. */
int mi355_xengine_xcorrelate_grouped_dev(mi355_xengine *h, const void *in_dev, void *out_dev, int accumulate,
                                         int stations_per_group, void *stream);
/* Batched form: nint integration windows in ONE launch -- what the worker thread of the reference does one window at a time
 * (the per-integration loop of lib/clXEngine_impl.cc:1234-1299).  in_dev holds nint windows back to back, each in the reference's
 * frame layout (stations_per_group == 0 or num_inputs), or -- the receive buffer of one all-to-all over nint windows --
 * [group][window][t][station in group][chan][pol]; out_dev receives nint matrices back to back (accumulate: each += its window).
 * With few channels per device (the channel slab of one rank of an 8-GPU X-engine) one window cannot fill the device and pays two
 * dispatches; a batch runs (window x column slice x time range) workgroups, and once nint * slices >= CUs no partial sums at all.
 * Other sample formats / geometries run the windows one after the other (group-major input of several windows: UNSUPPORTED). */
int mi355_xengine_xcorrelate_n_dev(mi355_xengine *h, int nint, const void *in_dev, void *out_dev, int accumulate,
                                   int stations_per_group, void *stream);
/* Which kernels the handle's LAST device-side call ran (no counterpart in the reference, whose one kernel per data type is fixed at construction,
 * lib/clXEngine_impl.cc:605-916): the routes differ 2 x in speed and depend on geometry, alignment, window count and environment switches, so a
 * caller (and the tests) can assert the one it expects.  The first use of a route on a handle is also logged at MI355_LOG_DEBUG. */
typedef struct mi355_xe_route {
    char kernel[64];          /* e.g. "k_xe_i8_lines", "k_xe_i8_lines<split>", "k_xe_i8_fused", "k_xe_i8_fused+k_xe_i8_reduce", "k_xe_turn_lds+k_xe_corr_sb" */
    int launches;             /* launches the last call was cut into (mi355_xengine_xcorrelate_n_dev splits window counts between the good ones) */
    int windows;              /* integration windows of the last launch */
    int workgroups;           /* of the last launch (0: not recorded for this route) */
    int units_per_workgroup;  /* persistent forms: units a workgroup runs one after the other */
    int tsplit;               /* time ranges per window (1: none) */
    int in_launch_reduce;     /* the time ranges are combined by the kernel's own tail (0: by a second kernel, or no ranges) */
    int touches;              /* early touches of the slow lines: distance in K blocks (0: off) */
    int pace;                 /* pacing of a line's workgroups, half K blocks (0: off) */
} mi355_xe_route;
int mi355_xengine_last_route(const mi355_xengine *h, mi355_xe_route *out);
/* Double-buffered asynchronous form of the host path: replaces the reference's pinned double
 * buffers + worker thread (lib/clXEngine_impl.cc:304-382 start(), :1234-1299 runThread()).
 * submit() copies the integration window into a pinned slot and enqueues H2D + kernels + D2H on that
 * slot's stream (acc_host != NULL: out = acc + V, pipeline integration); at most two are in flight.
 * wait() blocks for the OLDEST one and writes its matrix. */
int mi355_xengine_submit(mi355_xengine *h, const void *in_host, const void *acc_host);
int mi355_xengine_wait(mi355_xengine *h, void *out_host);
int mi355_xengine_pending(const mi355_xengine *h);
/* Zero-copy form of submit(): acquire() hands out the pinned frame buffer of the next free slot (input_bytes() long, the
 * reference's pinned char_input / complex_input, lib/clXEngine_impl.cc:325-362); the block gathers its frames straight
 * into it (mi355_xengine_gather or its own copies) and submit_acquired() enqueues H2D + kernels + D2H.  MI355_ERR_STATE
 * when two integrations are in flight.  Between acquire() and submit_acquired() a plain submit() is refused. */
int mi355_xengine_acquire(mi355_xengine *h, void **frame_buffer);
int mi355_xengine_submit_acquired(mi355_xengine *h, const void *accumulator_or_null);
/* host gather: copy frames [0,nframes) of each input stream into time slots
 * frame0.. of a frame buffer laid out as the reference's pinned host buffer */
int mi355_xengine_gather(const mi355_xengine *h, int nframes, int frame0, const void *const *inputs, void *frame_buffer);
/* ---- clXEngine over several devices of ONE process.  The reference picks one device per block (devId,
 * lib/GRCLBase.cpp:115-134) and a GNU Radio flowgraph is one process: this handle owns `world` device contexts and runs the FX correlator's
 * corner turn between them.  Rank r = device_ids[r] (a device may appear more than once: the ranks then share it) ingests antenna group r --
 * frames [window][t][num_inputs/world stations][chan][pol]{I,Q}, the reference's frame layout of lib/clXEngine_impl.cc:987-1061 -- and
 * produces channels [r F/W, (r+1) F/W) of the reference's [chan][baseline][pol^2] matrix (:786-808) for each of `windows` integration
 * windows per exchange.  IChar (int8 I/Q) with num_inputs * npol <= 64 rows, or 64 inputs x 2 polarisations with channel slabs of whole 32-channel
 * lines and enough windows per exchange to fill the device (8 ranks x 1024 channels: 8); world must divide num_inputs and num_channels.
 * Per exchange: one strided device copy packs a rank's frames into per-destination blocks (mi355_pack3d_dev), `world` peer copies
 * (hipMemcpyPeerAsync: xGMI) deliver them, and mi355_xengine_xcorrelate_n_dev reads the receive buffer in place; two slots, an exchange and
 * a compute stream per rank, so exchange k+1 runs under correlation k.  (gr-clenabled_amd/shard.py is the same pipeline with one process per
 * device and an RCCL all-to-all.) */
typedef struct mi355_xengine_shard mi355_xengine_shard;
int mi355_xengine_shard_create(int world, const int *device_ids, int npol, int num_inputs, int num_channels, int integration, int windows,
                               mi355_xengine_shard **out);
int mi355_xengine_shard_destroy(mi355_xengine_shard *h);
int mi355_xengine_shard_world(const mi355_xengine_shard *h);
int mi355_xengine_shard_device(const mi355_xengine_shard *h, int rank);
size_t mi355_xengine_shard_frames_bytes(const mi355_xengine_shard *h);  /* bytes of one rank's frames per exchange */
size_t mi355_xengine_shard_slab_items(const mi355_xengine_shard *h);    /* complex floats of one rank's matrix per window */
void *mi355_xengine_shard_stream(mi355_xengine_shard *h, int rank);     /* the rank's compute stream (hipStream_t): producers of frames_dev go here */
/* the rank's compute stream waits for everything enqueued so far on `stream` (hipStream_t of that device): the other way to order a producer */
int mi355_xengine_shard_wait_stream(mi355_xengine_shard *h, int rank, void *stream);
/* enqueue one exchange + correlation: frames_dev[r] / out_dev[r] live on device_ids[r] (out: windows x slab_items complex floats);
 * submit only ENQUEUES, so the packing copy of this exchange may still be reading frames_dev[r] after the next submit has returned: rewrite a
 * rank's frames only from work enqueued on mi355_xengine_shard_stream(rank) AFTER that next submit (it is ordered behind the next correlation,
 * which is behind this exchange's copies), or after mi355_xengine_shard_synchronize -- a producer on any other stream is not ordered behind the
 * pack.  An error return may leave the exchange half enqueued: synchronize and resubmit. */
int mi355_xengine_shard_submit_dev(mi355_xengine_shard *h, const void *const *frames_dev, void *const *out_dev, int accumulate);
int mi355_xengine_shard_synchronize(mi355_xengine_shard *h);
/* host form: `windows` windows in the reference's layout [window][t][station][chan][pol] -> [window][chan][baseline][pol^2]; every rank
 * copies its antenna group over its own host link and its slab back; blocking (lib/clXEngine_impl.h:179-201 over `world` devices) */
int mi355_xengine_shard_xcorrelate(mi355_xengine_shard *h, const void *in_host, void *out_host, int accumulate);
/* Streaming host form -- what a block that gathers frames all the time uses; the sharded counterpart of mi355_xengine_acquire / submit_acquired /
 * wait, i.e. of the reference's pinned frame buffers (lib/clXEngine_impl.cc:325-362) and worker thread (:1234-1299).  acquire(): a PINNED buffer of
 * input_bytes() = `windows` integration windows in the reference's frame layout, to be filled by the caller (mi355_xengine_gather writes this
 * layout); submit_acquired(): per rank, on the rank's own stream, the asynchronous upload of its antenna group out of that buffer (W host links at
 * once), exchange, correlation, download of its slab into a pinned result -- enqueue only; wait(): blocks for the OLDEST exchange, writes `windows`
 * matrices [window][chan][baseline][pol^2].  Two exchanges may be in flight (MI355_ERR_STATE beyond that), so the gather and upload of exchange
 * k+1 overlap the devices' work on exchange k. */
int mi355_xengine_shard_windows(const mi355_xengine_shard *h);
size_t mi355_xengine_shard_input_bytes(const mi355_xengine_shard *h);
int mi355_xengine_shard_acquire(mi355_xengine_shard *h, void **frame_buffer);
int mi355_xengine_shard_submit_acquired(mi355_xengine_shard *h);
int mi355_xengine_shard_wait(mi355_xengine_shard *h, void *out_host);
int mi355_xengine_shard_pending(const mi355_xengine_shard *h);
/* Self-test of the IChar scale (lib/clXEngine_impl.cc:859-867: every sample / 127, i.e. every sum / 16129): the device evaluates the
 * single-precision form the matrix stores use and the double expression (float)((double)S * (1/127) * (1/127)) for EVERY sum S with
 * |S| <= 2^24 (the range the single-precision form is used in) and counts the sums where the two floats differ; *mismatches must be 0. */
int mi355_xengine_selftest_scale(mi355_ctx *ctx, long long *mismatches);

/* ---------------------------------------------------------------------------
 * Remaining elementwise family.  One handle type; `kind` selects the block:
 *   LOG10       float -> float            c = p0*log10(a) + p1            clLog   (lib/clLog_impl.cc:113-147)
 *   SNR         float,float -> float      c = |p0*log10(a/b) + p1|        clSNR   (lib/clSNR_impl.cc:98-116)
 *   C2MAG       complex -> float          sqrt(im^2+re^2)                 clComplexToMag (:138-148)
 *   C2ARG       complex -> float          (float)atan2((double)im,(double)re)   clComplexToArg (:136-151)
 *   C2MAGPHASE  complex -> float,float    both of the above               clComplexToMagPhase (:150-164)
 *   MAGPHASE2C  float,float -> complex    (mag*cos ph, mag*sin ph) in double    clMagPhaseToComplex (:170-191)
 *   QUADDEMOD   complex -> float          p0*atan2(a[i+1]*conj(a[i])) in double, input carries 1 item of
 *                                         history (set_history(2))        clQuadratureDemod (:81,118-146)
 * Unused in/out pointers are NULL.  n = output items.
 * ------------------------------------------------------------------------- */
#define MI355_ELEM_LOG10      1
#define MI355_ELEM_SNR        2
#define MI355_ELEM_C2MAG      3
#define MI355_ELEM_C2ARG      4
#define MI355_ELEM_C2MAGPHASE 5
#define MI355_ELEM_MAGPHASE2C 6
#define MI355_ELEM_QUADDEMOD  7
int mi355_elem_create(mi355_ctx *ctx, int kind, float p0, float p1, mi355_elem **out);
int mi355_elem_destroy(mi355_elem *h);
int mi355_elem_history(const mi355_elem *h);
int mi355_elem_work(mi355_elem *h, size_t n, const void *in0, const void *in1, void *out0, void *out1);
int mi355_elem_work_dev(mi355_elem *h, size_t n, const void *in0, const void *in1, void *out0, void *out1, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Frequency-domain cross-correlator, replaces clxcorrelate_fft_vcf:
 *   make(fftSize, num_inputs, openCLPlatformType, devSelector, platformId, devId, input_type)
 *                                                  include/clenabled/clxcorrelate_fft_vcf.h:50
 *   work(): lib/clxcorrelate_fft_vcf_impl.cc:1058-1143.
 * Input 0 is the reference signal.  For every frame (vector of fft_size complex items) and every other
 * input s = 1..num_inputs-1:
 *     out[s-1][frame] = halfswap( | IFFT_unscaled( X0 * conj(Xs) ) | )        (float, fft_size items)
 * where X = the input itself (input_type 1, spectra) or its forward FFT (input_type 2, time series) and
 * halfswap exchanges the two halves of the vector (:1133-1140).  inputs[] holds num_inputs pointers to
 * [nframes][fft_size] complex, outputs[] num_inputs-1 pointers to [nframes][fft_size] float.
 * fft_size: powers of two 16..4096 run as ONE fused kernel; every other even size up to 4194304 (the reference hands fftSize to
 * clFFT, lib/clxcorrelate_fft_vcf_impl.cc:711-737) runs the reference's steps one after the other over the clFFT transforms of
 * this library; an odd size is refused (the reference would leave the last output of every vector unwritten).  num_inputs 2..32.
 * Reach: frame f of output s-1 depends on frame f of input 0 and frame f of input s alone -- not on the other frames of the call (however
 * many frames share a workgroup, wherever the frame sits in the call, whether its group is full or ragged), not on the other signals, and
 * not on how many signals the call has: a two-input call of (input 0, input s) gives the same bits.  A non-finite item in frame f of input
 * s >= 1 makes every lag of frame f of output s-1 non-finite; one in frame f of input 0 does that to frame f of every output; every other
 * frame of every output keeps its bits.  A frame in which either operand is all zero (spectra: also operands whose supports do not meet)
 * comes out as exact zeros.  work() gives the bits of work_device() (tests/test_xcorr_bounds_gpu.py).
 * ------------------------------------------------------------------------------------------------ */
int mi355_xcorr_fft_create(mi355_ctx *ctx, int fft_size, int num_inputs, int input_type, mi355_xcorr_fft **out);
int mi355_xcorr_fft_destroy(mi355_xcorr_fft *h);
int mi355_xcorr_fft_work(mi355_xcorr_fft *h, int nframes, const void *const *inputs, void *const *outputs);
int mi355_xcorr_fft_work_dev(mi355_xcorr_fft *h, int nframes, const void *const *d_inputs, void *const *d_outputs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Time-domain lag-search correlator, replaces clXCorrelate (all lines: lib/clXCorrelate_impl.cc):
 *   make(openCLPlatformType, devSelector, platformId, devId, setDebug, num_inputs, signal_length, data_type, data_size,
 *        max_search_index, decim_frames, async=false)            include/clenabled/clXCorrelate.h:55-56, ctor :700-747
 * data_type 1 (complex, data_size 8: magnitudes sqrtf(fmaf(re, re, im*im)), :915) or 2 (float, data_size 4: raw values).
 * Effective max shift M (:716-747): signal_length and max_search_index even; max_search_index <= 0 takes (int)(0.7*N) rounded
 * up to even; then rounded up to a power of two (M may reach or exceed N).  Limits here: num_inputs 2..32, signal_length
 * 2..2^24, M <= 2^24; anything else is an error (the reference exit(1)s).
 * Per frame of N items and per input s >= 1 (x = input 0, y = input s), g = 0 .. 2M-1, shift = g - M (kernel :851-899):
 *     curve[g] = sum_j x[j+shift] y[j] / sqrt(sum x^2 * sum y^2)    sums over the overlap 0 <= j, j+shift < N
 *     curve[g] = -2                                               if that energy product is 0 (no overlap included)
 *     corr = max curve, lag = argmax - M                            (find_max :1014-1045; ties go to the lowest g, non-finite
 *                                                                    entries never win; none finite: NaN and lag -M)
 * A copy of x delayed by d samples gives lag -d.  The PDU of the block (:1594-1600) carries corr / lag of every s >= 1.
 *   _plan       validation and rounding only (no device): *max_shift = M
 *   _work       one frame, host pointers inputs[num_inputs] of N items, blocking; corr / lags: num_inputs-1 values
 *   _submit / _poll / _wait   the async form (:1601-1645): submit enqueues one frame on the handle's stream and returns; poll
 *               returns 1 (result copied out) or 0 (still running); wait blocks until the submission has finished (poll
 *               then returns 1).  One submission at a time: submit or work with a result not yet polled is MI355_ERR_STATE.
 *   _work_dev   d_inputs[k] -> [nframes][N] items; d_corr, d_lags -> [nframes][num_inputs-1]; d_curves (or NULL) ->
 *               [nframes][num_inputs-1][2M] floats.  Two kernel launches per call (a call needing more than 256 MiB of
 *               workspace is cut into several pairs); the result of a frame does not depend on how frames are batched.
 * ------------------------------------------------------------------------------------------------ */
int mi355_xcorr_td_plan(int signal_length, int max_search_index, int *max_shift);
int mi355_xcorr_td_create(mi355_ctx *ctx, int num_inputs, int signal_length, int data_type, int data_size, int max_search_index,
                          mi355_xcorr_td **out);
int mi355_xcorr_td_destroy(mi355_xcorr_td *h);
int mi355_xcorr_td_max_shift(const mi355_xcorr_td *h);
int mi355_xcorr_td_work(mi355_xcorr_td *h, const void *const *inputs, float *corr, int *lags);
int mi355_xcorr_td_submit(mi355_xcorr_td *h, const void *const *inputs);
int mi355_xcorr_td_poll(mi355_xcorr_td *h, float *corr, int *lags);
int mi355_xcorr_td_wait(mi355_xcorr_td *h);
int mi355_xcorr_td_work_dev(mi355_xcorr_td *h, int nframes, const void *const *d_inputs, float *d_corr, int *d_lags,
                            float *d_curves, void *stream);

/* ------------------------------------------------------------------------------------------------
 * NCO / tone generator, replaces clSignalSource (lib/clSignalSource_impl.cc:113-237 kernels, 329-415 call), the fp64 branch:
 *   make(idataType, openCLPlatformType, devSelector, platformId, devId, samp_rate, waveform, freq, amplitude, setDebug=0)
 *                                                                               include/clenabled/clSignalSource.h:49-50
 * dtype COMPLEX, FLOAT or INT; waveform 1 (cos) or 2 (sin); samp_rate != 0 (anything else: MI355_ERR_INVALID_ARG).
 *     inc = 2 pi freq / samp_rate (double, 2 pi = 6.28318530717958647692);  A = (double)amplitude
 *     item i of a call:  d = pos + inc * (double)i
 *         complex  ((float)(cos d * A), (float)(sin d * A))         (whatever the waveform)
 *         float    (float)(cos d * A) or (float)(sin d * A), by waveform
 *         int      (int)(cos d * A) or (int)(sin d * A): evaluated in double and truncated toward zero (the reference's int
 *                  kernel does its phase arithmetic in float)
 *     after the call:  pos += inc * (double)(float)n;  if (pos > 2 pi || pos < -2 pi) pos = (pos/2pi - (double)(int)(pos/2pi)) * 2pi
 * pos is host state handed to the kernel as an argument: _work_dev calls are stream-ordered and keep no device state.  Complex
 * and float items are the float rounding of a double that is within a few double ulps of the formula (items off a thread's base
 * item are one rotation of it); int items evaluate the formula itself.
 *   _set_frequency keeps the phase; _set_phase sets pos; _get_state: pos and inc (either pointer may be NULL)
 *   _work       host pointer, blocking;  _work_dev: device pointer aligned to the item size, enqueue only.  n == 0: no-op.
 * Tuning aid, read once at _create: MI355_SIGSOURCE_LITERAL=1 evaluates every complex / float item literally (one sincos per item).
 * ------------------------------------------------------------------------------------------------ */
int mi355_sigsource_create(mi355_ctx *ctx, int dtype, double samp_rate, int waveform, double freq, float amplitude,
                           mi355_sigsource **out);
int mi355_sigsource_destroy(mi355_sigsource *h);
int mi355_sigsource_set_frequency(mi355_sigsource *h, double freq);
int mi355_sigsource_get_state(const mi355_sigsource *h, double *angle_pos, double *angle_rate);
int mi355_sigsource_set_phase(mi355_sigsource *h, double angle_pos);
int mi355_sigsource_work(mi355_sigsource *h, size_t n, void *out_host);
int mi355_sigsource_work_dev(mi355_sigsource *h, size_t n, void *out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------
 * BPSK / QPSK carrier recovery, replaces clCostasLoop (lib/clCostasLoop_impl.cc:112-232 kernel, 525-596 call), the fp64 + fma
 * branch:  make(openCLPlatformType, devSelector, platformId, devId, loop_bw, order, setDebug=0)   clCostasLoop.h:52
 * order 2 or 4 and loop_bw >= 0 (anything else: MI355_ERR_INVALID_ARG, the reference's invalid_argument at :80-83);
 * num_streams 1 .. 4096 (anything else: MI355_ERR_UNSUPPORTED).  Gains as gr::blocks::control_loop, in float, widened to double
 * (NOT cut to the six decimals of the reference's std::to_string, :136-137):
 *     damp = sqrt(2)/2;  denom = 1 + 2 damp bw + bw^2;  alpha = 4 damp bw / denom;  beta = 4 bw^2 / denom
 * Per stream the state (phase, freq, error) is three doubles in DEVICE memory, initially 0: consecutive calls chain with no host
 * round trip.  Per item (re, im), all in double:
 *     n_r = cos(-phase); n_i = sin(-phase)
 *     o_r = fma(re, n_r, -(im n_i));  o_i = fma(re, n_i, im n_r);   out = ((float)o_r, (float)o_i)
 *     e = order 2: o_r o_i;  order 4: (o_r > 0 ? 1 : -1) o_i - (o_i > 0 ? 1 : -1) o_r;      e = 0.5 (|e + 1| - |e - 1|)
 *     freq = fma(beta, e, freq);  phase = phase + fma(alpha, e, freq)
 *     if (phase > 2 pi || phase < -2 pi) phase = (phase/2pi - (double)(int)(phase/2pi)) * 2pi
 *     freq = clamp(freq, -1, 1);   freq_out (when given) = (float)freq
 * With several streams in / out / freq_out are item-major, stream s item i at [i * num_streams + s] (the channelizer's output
 * layout); num_streams = 1 is the reference's block.  Any split of a stream into consecutive calls gives bit-identical output.
 * Calls of one handle run in submission order, also when their streams differ (an event orders them).
 *   _plan       validation and gains only (no device)
 *   _get_state  num_streams doubles each (a NULL pointer is skipped); waits for the handle's last call
 *   _set_state  num_streams doubles each, NULL: left as it is; waits for the handle's last call
 *   _work       host pointers, blocking;  _work_dev: device pointers (in / out 8-byte, freq 4-byte aligned), enqueue only.
 *               in and out must not overlap (in == out is MI355_ERR_INVALID_ARG).  nitems == 0: no-op.
 * Tuning aid, read once at _create: MI355_COSTAS_ONE_LANE=1 runs a single stream through the several-streams kernel (one lane);
 * a handle's kernel never changes, so the bit-identity under splitting holds either way.
 * ------------------------------------------------------------------------------------------------ */
int mi355_costas_plan(float loop_bw, int order, float *alpha, float *beta);
int mi355_costas_create(mi355_ctx *ctx, float loop_bw, int order, int num_streams, mi355_costas **out);
int mi355_costas_destroy(mi355_costas *h);
int mi355_costas_set_loop_bandwidth(mi355_costas *h, float loop_bw);
int mi355_costas_get_state(mi355_costas *h, double *phase, double *freq, double *error);
int mi355_costas_set_state(mi355_costas *h, const double *phase, const double *freq);
int mi355_costas_work(mi355_costas *h, size_t nitems, const void *in, void *out, float *freq_out);
int mi355_costas_work_dev(mi355_costas *h, size_t nitems, const void *in_dev, void *out_dev, float *freq_dev, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Polyphase FIR with interpolation L and decimation M: clRationalResampler (M = 1: clInterpFIRFilter).  Beyond the reference
 * module, which has no resampler; the contract is GNU Radio's rational_resampler_ccf / ccc (interp_fir_filter_ccf / ccc at M = 1).
 * Taps h[0..K) real or complex, designed for L: L and M are used as given, NOT reduced by their gcd, and there is no gain
 * compensation (the taps carry the gain L).
 *     nt = ceil(K / L)   taps per arm = history();  hp = h zero-padded to nt L;  arm p = hp[p + L j], j = 0 .. nt-1
 * The input is complex64 and history-prefixed as clFilter's: in[nt-1] is x[0] of the call.  The handle's only state is the phase
 * c in [0, L), 0 at create, kept on the host (a kernel argument).  Output m = 0 .. n-1 of a call:
 *     q = c + m M;  p = q mod L;  b = q div L;     y[m] = sum_{j=0}^{nt-1} hp[p + L j] in[nt-1 + b - j]
 * and afterwards
 *     consumed = (c + n M) div L;  c' = (c + n M) mod L;  needed = n == 0 ? 0 : nt + (c + (n-1) M) div L   (items read)
 * The next call's `in` is this call's in + consumed.  All position arithmetic is 64-bit.  An output reads exactly the nt samples
 * in[b .. b+nt) and is one chain of float FMAs over them in an order fixed by its arm: any split of a stream into calls and any
 * 8-byte alignment of the buffers give the same bits.
 * Limits: 1 <= L, M <= 65536 and K >= 1 (smaller: MI355_ERR_INVALID_ARG, larger: MI355_ERR_UNSUPPORTED); nt L <= 1048576 table
 * entries (beyond: MI355_ERR_UNSUPPORTED, the reason in mi355_last_error()).
 *   _plan         the arithmetic above, no device (a block's forecast()); any output pointer may be NULL
 *   _noutput_for  largest n with needed(n) <= navail_with_history:
 *                 0 if navail < nt, else floor(((navail-nt+1) L - 1 - phase) / M) + 1;  a negative MI355_ERR_* on bad arguments
 *   _set_taps     keeps the phase; history() may change
 *   _set_phase    0 <= phase < L
 *   _work         host pointers, blocking (stages through device buffers of the handle)
 *   _work_dev     device pointers (8-byte aligned), enqueue only, allocates nothing
 *                 both advance the phase and report `consumed` (may be NULL); in and out must not overlap
 *                 (MI355_ERR_INVALID_ARG); noutput == 0 is a no-op.
 * Which kernel serves a handle is fixed at _create / _set_taps and named in that call's INFO line (debug contexts).
 * Tuning aids, read at _create / _set_taps: MI355_RESAMPLER_PLAIN=1 gives the handle the fallback kernel, MI355_RESAMPLER_GENERAL=1
 * the general kernel where the interpolation kernel would serve (comparison variants; all three give the same bits).
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_resampler mi355_resampler;
int mi355_resampler_plan(int interpolation, int decimation, int ntaps, int phase, long long noutput, int *taps_per_arm,
                         long long *consumed, long long *needed, int *phase_after);
long long mi355_resampler_noutput_for(int interpolation, int decimation, int ntaps, int phase, long long navail_with_history);
int mi355_resampler_create(mi355_ctx *ctx, int interpolation, int decimation, const void *taps, int ntaps, int complex_taps,
                           mi355_resampler **out);
int mi355_resampler_destroy(mi355_resampler *h);
/* takes effect at the next call; calls already enqueued keep what they were given */
int mi355_resampler_set_taps(mi355_resampler *h, const void *taps, int ntaps);
int mi355_resampler_ntaps(const mi355_resampler *h);
int mi355_resampler_get_taps(const mi355_resampler *h, void *taps_out, int cap);
int mi355_resampler_history(const mi355_resampler *h);
int mi355_resampler_get_phase(const mi355_resampler *h, int *phase);
int mi355_resampler_set_phase(mi355_resampler *h, int phase);
int mi355_resampler_work(mi355_resampler *h, long long noutput, const void *in_with_history, void *out, long long *consumed);
int mi355_resampler_work_dev(mi355_resampler *h, long long noutput, const void *in_with_history, void *out, long long *consumed,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * Polyphase synthesis bank: clPolyphaseSynthesizer, the counterpart of clPolyphaseChannelizer (mi355_pfb_*) in its critically
 * sampled form.  Beyond the reference module, which has no synthesizer; the role is that of GNU Radio's pfb_synthesizer_ccf at one
 * sample per channel per frame (no sample-for-sample parity with it is claimed; this comment is the contract).
 *     M = num_channels;  K = ntaps real taps g[0..K);  T = ceil(K / M) taps per arm;  g zero-padded to T M
 *     ch_map[0..nmap): input slot q feeds channel ch_map[q]; 1 <= nmap <= M, entries in [0, M) and distinct (a duplicate is
 *     MI355_ERR_INVALID_ARG); channels no slot feeds are zero.  ch_map == NULL: slot q feeds channel q.
 * The input is one complex64 stream of item-major frames of nmap items, U_f[q] = in[f nmap + q] -- what mi355_pfb_work_dev writes --
 * and history-prefixed: T - 1 old frames come first.  A call for nframes frames reads (T - 1 + nframes) nmap items and writes
 * nframes M items; l = 0 .. nframes-1, r = 0 .. M-1:
 *     V_f[r]     = sum_q U_f[q] exp(+2 pi i r ch_map[q] / M)               (backward DFT, scale 1, as in the channelizer)
 *     y[l M + r] = sum_{p=0}^{T-1} g[r + M p] V_{(l + T - 1) - p}[r]       (one float FMA chain per component, p ascending from +0)
 * The next call's `in` is this call's in + nframes nmap.  No device state and no gain compensation: the taps carry the gain.  The
 * oversampled (2x) form is not offered.
 * Limits: 1 <= M <= 4096, K >= 1, T M <= 1048576, nframes >= 0; in and out 8-byte aligned and not overlapping.  Below a range:
 * MI355_ERR_INVALID_ARG; above: MI355_ERR_UNSUPPORTED with the reason in mi355_last_error().
 * Routes, fixed at _create / _set_taps and named by _route() ("fused pow2 M=64 T=8 tile=64", "fused mixed-radix M=12 T=4 tile=64",
 * "generic"): one fused kernel (transform, then the FIR over frames that stay in LDS) for M = 8 .. 4096 a power of two and for
 * M = 2^a 3^b 5^c 7^d 11^e 13^f, as long as T - 1 frames fit the LDS ring; two kernels and a workspace of the handle otherwise.
 * A transformed frame does not depend on its place in a tile or a call and an output is one chain over exactly its T frames: any
 * split of a stream into calls and any 8-byte alignment give the same bits within a route; between routes the tolerance holds.
 * MI355_SYNTH_GENERIC=1, read at _create, gives the handle the generic route; MI355_SYNTH_TAPS_GLOBAL=1, read at _create / _set_taps,
 * makes the power-of-two kernel read its taps through the caches where they would fit the LDS (comparison variants, same bits; _route()
 * then ends in " taps=global").
 *   _plan      the arithmetic above, no device; any output pointer may be NULL
 *   _create    everything that can be told without a device is checked before ctx is touched
 *   _set_taps  may change T, and with it the history (T - 1) nmap
 *   _route     valid until the next _set_taps / _destroy of the handle
 *   _work      host pointers, blocking (stages through device buffers of the handle)
 *   _work_dev  device pointers, enqueue only (the generic route sizes its workspace on the first call); nframes == 0 is a no-op
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_synth mi355_synth;
int mi355_synth_plan(int ntaps, int num_channels, int nmap, long long nframes, int *taps_per_arm, long long *ninput_items,
                     long long *noutput_items);
int mi355_synth_create(mi355_ctx *ctx, const float *taps, int ntaps, int num_channels, const int *ch_map, int nmap, mi355_synth **out);
int mi355_synth_destroy(mi355_synth *h);
/* takes effect at the next call; calls already enqueued keep what they were given */
int mi355_synth_set_taps(mi355_synth *h, const float *taps, int ntaps);
int mi355_synth_ntaps(const mi355_synth *h);
int mi355_synth_get_taps(const mi355_synth *h, float *taps_out, int cap);
int mi355_synth_taps_per_arm(const mi355_synth *h);
int mi355_synth_num_channels(const mi355_synth *h);
int mi355_synth_nmap(const mi355_synth *h);
const char *mi355_synth_route(const mi355_synth *h);
int mi355_synth_work(mi355_synth *h, long long nframes, const void *in_with_history, void *out);
int mi355_synth_work_dev(mi355_synth *h, long long nframes, const void *in_with_history, void *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Averaged power spectrum: clPowerSpectrum, window + forward DFT + |X|^2 + mean over K frames (+ dB) in one block.  Beyond the
 * reference module, which has no spectrum estimator; the role is that of GNU Radio's logpwrfft and of the Bartlett / Welch
 * periodogram (this comment is the contract).
 *     N = fft_size;  w[0..N) = window (NULL / window_len 0: all ones; window_len must be N or 0);  K = navg >= 1 frames per spectrum;
 *     H = hop >= 1 items from the start of one frame to the start of the next: H = N Bartlett, H < N Welch overlap, H > N skips
 *     items (logpwrfft's frame-rate decimation; the skipped items are never read);  shift, log_output: 0 or 1;  scale: float.
 * Input complex64 x, output float32; spectrum s = 0 .. S-1, bin b = 0 .. N-1:
 *     P_s[b] = scale (1 / K) sum_{k < K} | DFT_N( w .* x[(s K + k) H + (0 .. N)) )[b] |^2        (forward DFT, unnormalised)
 * shift: the output is in fftshift order, out[i] = P[(i + ceil(N / 2)) mod N] -- clFFT's permutation, odd N included, which is
 * numpy's fftshift.  log_output: 10 log10(P) is written; P = 0 gives -inf, as in numpy.
 * Buffers: a call for S spectra reads exactly (S K - 1) H + N input items (none when S = 0) and writes exactly S N floats; `in` may
 * have any 8-byte and `out` any 4-byte alignment; a misaligned pointer, or in / out that overlap, is MI355_ERR_INVALID_ARG with nothing
 * launched.  The next call's `in` is this call's in + S K H; history() of the block is max(N - H, 0).
 * Routes, named by _route(): "fused pow2 N=1024 chunk=64" -- N = 16 .. 4096 a power of two: one kernel that keeps clFFT's transform in
 * registers, adds re^2 + im^2 over a chunk of C frames per workgroup and stores N floats per chunk (K <= C: the finished spectrum;
 * K > C: partial sums into a workspace of the handle, added in chunk order by a second, small kernel); "generic N=1000 batch=1048" --
 * every other length mi355_fft_create takes, and every handle under _set_generic(h, 1): an internal clFFT handle transforms bounded
 * batches of frames (gathered first when H != N) into a workspace and a second kernel adds |X|^2 over a spectrum's frames, k ascending.
 * The partition of K and the order of every sum are functions of (N, K) alone and no float atomics are used: the bits of a spectrum
 * depend neither on S nor on its place in the call, so any split of a stream into calls at spectrum boundaries, at any legal
 * alignment, gives the same bits within a route; between routes the tolerance holds.
 * Limits: N, K or H < 1, a window_len other than 0 or N: MI355_ERR_INVALID_ARG.  An N that mi355_fft_create would refuse (1, or above
 * its range): MI355_ERR_UNSUPPORTED with clFFT's reason in mi355_last_error().  Item counts are long long; above 2^62 (_plan) or 2^44
 * per call (_work, _work_dev): MI355_ERR_UNSUPPORTED.  Real input, exponential averaging across calls and one-sided output are not offered.
 *   _plan        the arithmetic above, no device; either output pointer may be NULL
 *   _create      everything that can be told without a device is checked before ctx is touched
 *   _set_scale, _set_window   take effect at the next call; calls already enqueued keep what they were given
 *   _set_generic on != 0: the generic route for every later call of the handle (there is no environment switch); 0: back
 *   _route       valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _work        host pointers, blocking (stages whole spectra through device buffers of the handle)
 *   _work_dev    device pointers, enqueue only; nspectra == 0 is a no-op.  Calls that use the handle's workspace (K > C, generic)
 *                from different streams are accepted and ordered on it; use one handle per stream for overlap.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_pspec mi355_pspec;
int mi355_pspec_plan(int fft_size, int navg, int hop, long long nspectra, long long *ninput_items, long long *noutput_items);
int mi355_pspec_create(mi355_ctx *ctx, int fft_size, const float *window, int window_len, int navg, int hop, int shift, int log_output,
                       float scale, mi355_pspec **out);
int mi355_pspec_destroy(mi355_pspec *h);
int mi355_pspec_set_scale(mi355_pspec *h, float scale);
int mi355_pspec_set_window(mi355_pspec *h, const float *window, int window_len);
int mi355_pspec_set_generic(mi355_pspec *h, int on);
int mi355_pspec_fft_size(const mi355_pspec *h);
int mi355_pspec_navg(const mi355_pspec *h);
int mi355_pspec_hop(const mi355_pspec *h);
const char *mi355_pspec_route(const mi355_pspec *h);
int mi355_pspec_work(mi355_pspec *h, long long nspectra, const void *in, void *out);
int mi355_pspec_work_dev(mi355_pspec *h, long long nspectra, const void *in, void *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Frequency-translating FIR filter: clFreqXlatingFIRFilter, tune + low-pass + decimate for C channels of one wideband stream.  Beyond
 * the reference module; the contract is GNU Radio's freq_xlating_fir_filter_ccf / ccc (this comment is the contract).
 *     h[0..K) = prototype taps (float, or complex64 with complex_taps != 0);  D = decimation >= 1;  fs = samp_rate > 0;
 *     f_c = center_freqs[c], c = 0 .. C-1, C = nfreq >= 1.  All channels share h and D.
 * Input: GNU Radio's history-prefixed buffer of complex64, in[K-1] is x[0]; a call for n outputs reads exactly n D + K - 1 items (none
 * when n = 0) and writes exactly n complex64 items to each of the C buffers outs[0..C).  Output m (counted since create) of channel c:
 *     y_c[m] = r_c(m) sum_k b_c[k] x[m D - k]
 *     b_c[k] = h[k] exp(+j 2 pi frac(k f_c / fs))        float64 on the host, rounded to float32 (_get_bandpass_taps)
 *     r_c(m) = exp(-j 2 pi P_c(m) / 2^64),   P_c(m) = (P_c(0) + inc_c m) mod 2^64,    inc_c = round(frac(f_c D / fs) 2^64) mod 2^64
 * (inc_c is evaluated on the signed fraction nearest zero, so -f gives exactly 2^64 - inc.)
 * -- band-pass taps, decimate, rotate by -omega D per output, which is mixing x down by f_c, filtering with h and decimating.  The
 * phase is a 64-bit fixed-point accumulator kept on the host per channel (P_c = 0 at create, advanced by inc_c n after a call of n
 * outputs) and evaluated on the device in integer arithmetic per output, then one double sincospi, rounded to float: nothing drifts at
 * any stream length, and _set_center_freq keeps P_c (the phase is continuous across a retune; inc_c and b_c are rebuilt).
 * Routes, named by _route() and decided at _create / _set_taps from (D, K, C) alone: "fused D=16 K=65 C=8 tile_out=128" -- D = 2 .. 64,
 * K <= 512, C <= 16 and taps + tile within 160 KiB of LDS: one kernel that stages a tile's input span once and forms the outputs of all
 * C channels from it; "generic D=1 K=3000 C=20" -- everything else, and every handle under _set_generic(h, 1): per channel an internal
 * clComplexFilter handle (taps b_c, decimation D, the use_time given here) and an in-place rotate kernel with the same integer phase.
 * Fused route: any split of a stream into calls and any 8-byte alignment of `in` / outs[c] give the same bits.  Generic route: the bits
 * are clComplexFilter's, rotated -- the same for any split as long as clComplexFilter picks the same kernel (direct form: it looks at
 * the 16-byte alignment of `in`; overlap-save blocks start at a call's first output).  Between routes the tolerance holds.
 * Errors (nothing launched): NULL pointers, `in` or an outs[c] not 8-byte aligned, `in` overlapping an output, nfreq < 1, samp_rate
 * <= 0 or not finite, a frequency that is not finite, c out of range: MI355_ERR_INVALID_ARG.  More than 4096 channels, more than 2^62
 * items (_plan) or 2^44 input items per call: MI355_ERR_UNSUPPORTED.
 *   _plan         ninput_items = noutput D + K - 1 (0 for no output), history = K (GNU Radio's set_history(K)); no device; either
 *                 output pointer may be NULL
 *   _create       everything that can be told without a device is checked before ctx is touched
 *   _set_taps     new prototype (same kind as at create), any length; phases are kept; the route is decided again
 *   _get_taps / _get_bandpass_taps   return K; cap counts taps; the band-pass taps are complex64 whatever the prototype
 *   _get_state    P_c of the next output and inc_c (either pointer may be NULL);  _set_phase sets P_c
 *   _skip         advances every P_c as if noutputs outputs had been made, no device work (dropped upstream samples, resuming a stream)
 *   _set_generic  on != 0: the generic route for every later call of the handle (there is no environment switch); 0: back
 *   _route        valid until the next _set_generic / _set_taps / _destroy of the handle; "" for NULL
 *   _work         host pointers, blocking (pieces staged through pinned buffers of the handle)
 *   _work_dev     device pointers (outs: a host array of C device pointers), enqueue only; noutput == 0 is a no-op
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_xlate mi355_xlate;
int mi355_xlate_plan(int decimation, int ntaps, long long noutput, long long *ninput_items, int *history);
int mi355_xlate_create(mi355_ctx *ctx, int decimation, const void *taps, int ntaps, int complex_taps, double samp_rate,
                       const double *center_freqs, int nfreq, int use_time, mi355_xlate **out);
int mi355_xlate_destroy(mi355_xlate *h);
/* takes effect at the next call; calls already enqueued keep what they were given */
int mi355_xlate_set_taps(mi355_xlate *h, const void *taps, int ntaps);
int mi355_xlate_ntaps(const mi355_xlate *h);
int mi355_xlate_get_taps(const mi355_xlate *h, void *taps_out, int cap);
int mi355_xlate_num_channels(const mi355_xlate *h);
int mi355_xlate_decimation(const mi355_xlate *h);
/* takes effect at the next call; calls already enqueued keep what they were given */
int mi355_xlate_set_center_freq(mi355_xlate *h, int c, double freq);
int mi355_xlate_get_center_freq(const mi355_xlate *h, int c, double *freq);
int mi355_xlate_get_bandpass_taps(const mi355_xlate *h, int c, void *out, int cap);
int mi355_xlate_get_state(const mi355_xlate *h, int c, unsigned long long *phase, unsigned long long *inc);
int mi355_xlate_set_phase(mi355_xlate *h, int c, unsigned long long phase);
int mi355_xlate_skip(mi355_xlate *h, long long noutputs);
int mi355_xlate_set_generic(mi355_xlate *h, int on);
const char *mi355_xlate_route(const mi355_xlate *h);
int mi355_xlate_work(mi355_xlate *h, long long noutput, const void *in_with_history, void *const *outs);
int mi355_xlate_work_dev(mi355_xlate *h, long long noutput, const void *in_with_history, void *const *outs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Tied-array beamformer: clBeamformer, B beams from the S inputs of the X-engine's int8 frames, per channel a complex int8 weight
 * matrix, delivered as voltage beams or as detected, time-integrated power.  Beyond the reference module, which has no beamformer
 * (this comment is the contract).  Both modes are integer-exact: there is no tolerance anywhere.
 *     mode = MI355_BEAMFORM_VOLTAGE (0) or MI355_BEAMFORM_POWER (1);  npol = 1 or 2;  S = num_inputs 1 .. 512;  F = num_channels >= 1;
 *     B = num_beams 1 .. 1024;  Ti = integration 1 .. 4096 (POWER only, it must be 1 for VOLTAGE);  stokes_i = 0 or 1 (POWER only, and
 *     it needs npol = 2).
 * Input: the X-engine's BYTE frame layout.  One frame is x[s][f][p] = int8 {I, Q}, frame_bytes = 2 S F npol, frames consecutive in
 * time; every int8 value is legal, -128 included.
 * Weights: w[f][p][b][s] = int8 {re, im}, 2 F npol B S bytes.  Every component must lie in -127 .. 127: a -128 is
 * MI355_ERR_INVALID_ARG (which lets a kernel negate a weight byte without overflow).  weights == NULL at _create means all zero.
 * VOLTAGE, for each frame t:
 *     y[t][b][f][p] = sum_s w[f][p][b][s] x[t][s][f][p]
 * a complex product in integer arithmetic, exact in int32: each component satisfies |component| <= S 2 127 128 <= 16 646 144 < 2^24
 * (the reason for S <= 512), so the complex64 output, layout [t][b][f][p], holds the exact integers.  The unit of work is one frame; a
 * unit writes B F npol complex64.
 * POWER, for each window W of Ti consecutive frames:
 *     P[W][b][f][p] = (float) sum_{t in W} (re^2 + im^2)
 * the sum taken exactly in int64 (bounded by 2 (1.67e7)^2 4096 2 = 4.6e18 < 2^63, the reason for Ti <= 4096) and converted to float32
 * once, round to nearest even.  With stokes_i the sum also runs over p and the output is [W][b][f].  The unit of work is one window; a
 * unit writes B F (stokes_i ? 1 : npol) floats.
 * Any split of a stream into calls at unit boundaries, any legal alignment and either route give identical bits.
 * Routes, decided at _create from the geometry alone and named by _route(): "mfma S=64 B=64 F=1024 npol=2 kblocks=2 beam_tiles=4" --
 * F npol 2 a multiple of 16 and S <= 256 (any B): per (f, p) the product (B x S) . (S x time) on v_mfma_i32_16x16x64_i8 with K = the
 * interleaved (station, {I, Q}) bytes, zero padded in registers (nothing past a frame is read); "generic S=3 B=2 F=5 npol=1" --
 * everything else, every handle under _set_generic(h, 1), and any single call whose `in` is not 16-byte aligned: one thread per output,
 * the same integer arithmetic.  The route is forced by _set_generic only; there is no environment switch.
 * Weight updates: a call enqueued before _set_weights / _set_beam_weights returns uses the old weights entirely, a later call the new
 * ones entirely (versioned device buffers; an old version is released behind the event of its last launch, when the next update or
 * _destroy finds it complete; nothing on the work path waits for the device).
 * Errors (nothing launched): NULL pointers, `in` not 2-byte aligned, `out` not 8-byte (VOLTAGE) / 4-byte (POWER) aligned, `in`
 * overlapping `out`, a parameter outside the ranges above, a weight of -128, `beam` out of range: MI355_ERR_INVALID_ARG.  More than 2^40
 * input bytes per call, or a weight set above 2 GiB: MI355_ERR_UNSUPPORTED.
 *   _plan         frame_bytes, frames_per_unit (Ti; 1 for VOLTAGE), out_bytes_per_unit; no device; any output pointer may be NULL
 *   _create       everything that can be told without a device is checked before ctx is touched
 *   _set_weights  replaces all weights;  _set_beam_weights: those of one beam, w_beam = [f][p][s] {re, im}
 *   _get_weights  copies the 2 F npol B S weight bytes; cap_bytes is the size of `out`
 *   _set_generic  on != 0: the generic route for every later call of the handle; 0: back
 *   _route        valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _work         host pointers, blocking (pieces of whole units staged through pinned buffers of the handle)
 *   _work_dev     device pointers, enqueue only; nunits == 0 is a no-op
 * ------------------------------------------------------------------------------------------------ */
#define MI355_BEAMFORM_VOLTAGE 0
#define MI355_BEAMFORM_POWER 1
typedef struct mi355_beamform mi355_beamform;
int mi355_beamform_plan(int mode, int npol, int num_inputs, int num_channels, int num_beams, int integration, int stokes_i,
                        long long *frame_bytes, int *frames_per_unit, long long *out_bytes_per_unit);
int mi355_beamform_create(mi355_ctx *ctx, int mode, int npol, int num_inputs, int num_channels, int num_beams, int integration,
                          int stokes_i, const void *weights, mi355_beamform **out);
int mi355_beamform_destroy(mi355_beamform *h);
int mi355_beamform_set_weights(mi355_beamform *h, const void *weights);
int mi355_beamform_set_beam_weights(mi355_beamform *h, int beam, const void *w_beam);
int mi355_beamform_get_weights(const mi355_beamform *h, void *out, long long cap_bytes);
int mi355_beamform_num_beams(const mi355_beamform *h);
long long mi355_beamform_frame_bytes(const mi355_beamform *h);
long long mi355_beamform_out_bytes_per_unit(const mi355_beamform *h);
int mi355_beamform_set_generic(mi355_beamform *h, int on);
const char *mi355_beamform_route(const mi355_beamform *h);
int mi355_beamform_work(mi355_beamform *h, long long nunits, const void *in, void *out);
int mi355_beamform_work_dev(mi355_beamform *h, long long nunits, const void *in, void *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * F-engine: clFEngine, polyphase filter bank + forward DFT + gain + int8 quantisation of R = S npol complex64 streams into the int8
 * frames that clXEngine (BYTE) and clBeamformer consume.  Beyond the reference module, which has no F-engine (this comment is the
 * contract).
 *     S = num_inputs (stations) 1 .. 4096;  npol = 1 or 2;  F = num_channels, any length mi355_fft_create takes (>= 2);
 *     P = taps_per_channel 1 .. 1024;  shift = 0 or 1 (1 needs an even F).
 * Input r = s npol + p is a complex64 stream.  taps: P F real float32 prototype taps h (NULL at _create: all ones); P = 1 is a
 * windowed FFT.  For frame t of input r:
 *     z[n] = sum_{p < P} h[p F + n] x_r[(t + p) F + n]                    n = 0 .. F-1
 *     X[f] = sum_n z[n] exp(-j 2 pi f n / F)
 *     v    = gain[r][f] X[f]                                              real float32 gain, [r][f]; NULL at _create: all 1
 *     q    = clamp(rint(v.re), -127, 127), clamp(rint(v.im), -127, 127)   rint = round half to even
 *     out[t][s][f'][p] = int8 {q.re, q.im},   f' = shift ? (f + F / 2) mod F : f       (f ^ (F / 2) when F is a power of two)
 * This is the critically sampled analysis bank of radio astronomy -- hop F, window P F, the taps applied in the order of the stream --
 * NOT the GNU Radio arm convention of clPolyphaseChannelizer (whose arms run against the stream and whose outputs are per-channel
 * streams).  Saturation is symmetric: -128 is never produced.  A NaN component becomes 0.  Every component that saturated or was NaN
 * adds one to the clip counter of its input r (uint64, integer atomics): the totals are exact and do not depend on how a stream is
 * split into calls.
 * Calling convention: in_with_history[r] points at the first item of the first frame's window; a call for n frames reads
 * (n + P - 1) F items per input and nothing beyond, and writes n frames of frame_bytes = 2 S F npol bytes.  The caller advances every
 * pointer by n F items between calls.  Any split of a stream into calls at frame boundaries and any legal alignment (inputs 8-byte,
 * out 2-byte) give the same bits within a route.
 * Routes, decided at _create and named by _route(): "fused pow2 F=1024 P=4 npol=2 group=4" -- F = 16 .. 4096 a power of two and
 * P <= 16: one kernel, the arms, the register transform of clFFT, gain, round, clamp and pack, whole rows out[t][s][.][.] stored 16
 * bytes at a time; "generic F=1000 P=4 npol=2 batch=32x65" -- every other F, P > 16 and every handle under _set_generic(h, 1): a
 * weighted-overlap-add kernel, an internal clFFT handle on a bounded workspace, a quantise-and-pack kernel.  The route is forced by
 * _set_generic only; there is no environment switch.  The two routes order their float32 sums differently: an output whose exact value
 * lies within the rounding error of a half-integer (or of +-127.5) may differ by one between them.
 * Gain updates: a call enqueued before _set_gains / _set_input_gain returns uses the old gains entirely, a later call the new ones
 * entirely (versioned device buffers; an old version is released behind the event of its last launch, when the next update or
 * _destroy finds it complete; nothing on the work path waits for the device).
 * Errors (nothing launched): NULL pointers, an input not 8-byte aligned, `out` not 2-byte aligned, an input overlapping `out`, a
 * parameter outside the ranges above, shift with an odd F, `input` out of range: MI355_ERR_INVALID_ARG.  An F that mi355_fft_create
 * would refuse, a gain or tap table above 1 GiB, more than 2^40 bytes per buffer and call: MI355_ERR_UNSUPPORTED.
 *   _plan            frame_bytes, history_items = (P - 1) F, items_per_input = nframes F + history (0 for no frames); no device; any
 *                    output pointer may be NULL
 *   _create          everything that can be told without a device is checked before ctx is touched
 *   _set_gains       replaces all gains, [r][f];  _set_input_gain: the F gains of one input;  _get_gains copies the R F floats
 *   _get_clips       waits for the device, copies the R counters to out; reset != 0 zeroes them afterwards
 *   _set_generic     on != 0: the generic route for every later call of the handle; 0: back
 *   _route           valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _work            host pointers, blocking (pieces of whole frames staged through buffers of the handle)
 *   _work_dev        device pointers (the pointer array itself lives on the host), enqueue only; nframes == 0 is a no-op
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_fengine mi355_fengine;
int mi355_fengine_plan(int num_inputs, int npol, int num_channels, int taps_per_channel, int shift, long long nframes,
                       long long *frame_bytes, long long *history_items, long long *items_per_input);
int mi355_fengine_create(mi355_ctx *ctx, int num_inputs, int npol, int num_channels, int taps_per_channel, const float *taps, int shift,
                         const float *gains, mi355_fengine **out);
int mi355_fengine_destroy(mi355_fengine *h);
int mi355_fengine_set_gains(mi355_fengine *h, const float *gains);
int mi355_fengine_set_input_gain(mi355_fengine *h, int input, const float *gain);
int mi355_fengine_get_gains(const mi355_fengine *h, float *out, long long cap_floats);
int mi355_fengine_get_clips(mi355_fengine *h, unsigned long long *out, int reset);
int mi355_fengine_set_generic(mi355_fengine *h, int on);
const char *mi355_fengine_route(const mi355_fengine *h);
long long mi355_fengine_frame_bytes(const mi355_fengine *h);
long long mi355_fengine_history_items(const mi355_fengine *h);
int mi355_fengine_work(mi355_fengine *h, long long nframes, const void *const *in_with_history, void *out);
int mi355_fengine_work_dev(mi355_fengine *h, long long nframes, const void *const *in_with_history, void *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Dedisperser: clDedisperser, exact incoherent dedispersion of a filterbank over D dispersion-measure trials -- the first stage of a
 * pulsar or fast-transient search behind clBeamformer's POWER output.  Beyond the reference module, which has no dedisperser (this
 * comment is the contract).  The summation order is pinned, so there is no tolerance anywhere.
 *     R = num_rows (beams) 1 .. 4096;  F = num_channels 1 .. 16384;  D = num_trials 1 .. 4096;  H = max_delay 0 .. 2^20, fixed for
 *     the life of the handle (it is the block's history);  order = MI355_DEDISP_TRIAL_MAJOR (0) or MI355_DEDISP_TIME_MAJOR (1).
 * Input: x[t][r][f] float32, channel fastest -- clBeamformer's POWER output with stokes_i = 1 or npol = 1 and B = R.  A call for n
 * outputs reads the n + H time samples that start at `in` and nothing beyond; the caller advances `in` by n R F floats between calls.
 * Delay table: delay[d][f] int32, D F entries, each in 0 .. H or -1.  -1 means "channel f takes no part in trial d" (a killed
 * channel): nothing of that channel is added, a NaN there reaches nothing.  Any other value is MI355_ERR_INVALID_ARG.  delays == NULL
 * at _create means all zero.
 * Output, for output sample t of the call:
 *     y(r, d, t) = (((+0.0f + x[t + delay[d][0]][r][0]) + x[t + delay[d][1]][r][1]) + ...)     skipping every f with delay[d][f] == -1
 * IEEE binary32 additions, round to nearest even, one rounding per addition, in ascending channel order.  The result is a function of
 * the inputs alone: either route, any split of a stream into calls, any legal alignment and any n give identical bits.  NaN and +-Inf
 * propagate exactly where the formula puts them and nowhere else.  Results whose operands or partial sums are subnormal are
 * unspecified.  (The fixed order rules out float atomics and any split of a channel sum across threads; the R D sums of a time sample
 * are the parallelism.)
 * Output layout: TRIAL_MAJOR y[(r D + d) out_pitch + t] with out_pitch >= n in floats; the floats between n and out_pitch are not
 * touched, so a caller fills long per-trial time series over several calls.  TIME_MAJOR y[t][r][d], out_pitch must be 0.
 * Routes, decided at _create and again at every _set_delays from the table, named by _route(): "tiled R=64 F=1024 D=1024 fb=8 dt=16
 * tt=256" -- a workgroup owns (row, dt trials, tt outputs), walks the channels in blocks of fb, stages per block only the window
 * [t0 + min delay, t0 + tt + max delay) of the (trial tile, channel block) in LDS transposed and keeps its accumulators in registers;
 * taken when max - min <= 128 in every (trial tile, channel block), -1 entries not counted, and R F <= 2796202 (a window of less than
 * 2^32 bytes).  "generic R=3 F=5 D=2" -- any other table
 * and every handle under _set_generic(h, 1): one thread per output.  The route is forced by _set_generic only; there is no
 * environment switch.  A _set_delays may change the route.
 * Table updates: a call enqueued before _set_delays returns uses the old table entirely, a later call the new one entirely (versioned
 * device buffers; an old version is released behind the event of its last launch, when the next update or _destroy finds it complete;
 * nothing on the work path waits for the device).  A refused update changes nothing.
 * Errors (nothing launched): NULL pointers, `in` or `out` not 4-byte aligned, `in` overlapping the extent of `out`, out_pitch < n
 * (TRIAL_MAJOR) or != 0 (TIME_MAJOR), a parameter outside the ranges above, a table entry outside -1 .. H: MI355_ERR_INVALID_ARG.
 * More than 2^40 bytes per buffer and call, or a table above 1 GiB: MI355_ERR_UNSUPPORTED.
 *   _plan         in_floats_per_sample = R F, history = H, out_floats_per_sample = R D; no device; any output pointer may be NULL
 *   _create       everything that can be told without a device is checked before ctx is touched
 *   _set_delays   replaces the whole table (validated against H);  _get_delays copies the D F entries, cap_entries is the size of `out`
 *   _history      H
 *   _set_generic  on != 0: the generic route for every later call of the handle; 0: back
 *   _route        valid until the next _set_generic / _set_delays / _destroy of the handle; "" for NULL
 *   _work         host pointers, blocking (pieces of whole samples, each staged with its H samples of look-ahead)
 *   _work_dev     device pointers, enqueue only; n == 0 is a no-op
 * mi355_dedisp_delays (host only, no context): the cold-plasma delay table of a band of F channels nu_f = f0 + f df MHz (df may be
 * negative) against the largest nu_f, for D dispersion measures in pc cm^-3 and a sampling time in seconds:
 *     delay[d][f] = llrint(((4.148808e3 dm[d]) (1 / (nu_f nu_f) - 1 / (nu_ref nu_ref))) / tsamp_s)
 * in double, every operation rounded on its own (never contracted), llrint in the default rounding mode (half to even).  *max_delay
 * (may be NULL) receives the largest entry.  A non-positive or non-finite nu_f, tsamp_s <= 0, a negative or non-finite dm or a delay
 * above 2^20: MI355_ERR_INVALID_ARG, and `out` is then unspecified.
 * ------------------------------------------------------------------------------------------------ */
#define MI355_DEDISP_TRIAL_MAJOR 0
#define MI355_DEDISP_TIME_MAJOR 1
typedef struct mi355_dedisp mi355_dedisp;
int mi355_dedisp_plan(int num_rows, int num_channels, int num_trials, int max_delay, int order, long long *in_floats_per_sample,
                      long long *history, long long *out_floats_per_sample);
int mi355_dedisp_create(mi355_ctx *ctx, int num_rows, int num_channels, int num_trials, int max_delay, int order, const int32_t *delays,
                        mi355_dedisp **out);
int mi355_dedisp_destroy(mi355_dedisp *h);
int mi355_dedisp_set_delays(mi355_dedisp *h, const int32_t *delays);
int mi355_dedisp_get_delays(const mi355_dedisp *h, int32_t *out, long long cap_entries);
long long mi355_dedisp_history(const mi355_dedisp *h);
int mi355_dedisp_set_generic(mi355_dedisp *h, int on);
const char *mi355_dedisp_route(const mi355_dedisp *h);
int mi355_dedisp_work(mi355_dedisp *h, long long n, const void *in, void *out, long long out_pitch);
int mi355_dedisp_work_dev(mi355_dedisp *h, long long n, const void *in, void *out, long long out_pitch, void *stream);
int mi355_dedisp_delays(double f0_mhz, double df_mhz, int num_channels, double tsamp_s, const double *dm, int num_trials, int32_t *out,
                        int *max_delay);

/* ------------------------------------------------------------------------------------------------
 * Pulse search: clPulseSearch, an exact boxcar single-pulse search over the R D dedispersed time series that clDedisperser delivers:
 * a bank of K boxcar matched filters of widths 2^0 .. 2^(K-1) per series, normalised to S/N, reduced to one peak per (block of Tb
 * outputs, series) and, optionally, to a list of the peaks at or above a threshold.  Beyond the reference module, which has no such
 * block (this comment is the contract).  The arithmetic is pinned, so there is no tolerance anywhere except in _measure.
 *     R = num_rows 1 .. 4096;  D = num_trials 1 .. 4096;  S = R D series, s = r D + d;  K = num_widths 1 .. 13;
 *     history (look-ahead) Hs = 2^(K-1) - 1;  Tb = block_len 16 .. 2^24 - 1, any integer;
 *     order = MI355_PSEARCH_TRIAL_MAJOR (0) or MI355_PSEARCH_TIME_MAJOR (1): the two output orders of clDedisperser, same values.
 * Input: float32.  TRIAL_MAJOR x[s in_pitch + t] with in_pitch >= n + Hs in floats; the floats between n + Hs and in_pitch are never
 * read.  TIME_MAJOR x[t][r][d], in_pitch must be 0.  A call for n outputs per series reads the n + Hs samples per series that start
 * at `in` and nothing beyond; n must be a multiple of Tb; n == 0 is a no-op.  Between calls the caller advances `in` by n samples.
 * Boxcar sums are a dyadic tree, and the tree is the contract:
 *     b_0[t] = x[t];     b_k[t] = b_(k-1)[t] + b_(k-1)[t + 2^(k-1)]
 * each one IEEE binary32 addition, round to nearest even, one rounding.  Every b_k[t] is a fixed balanced tree over x[t .. t + 2^k):
 * a function of those inputs alone, whatever the tiling.  (A left-to-right or prefix-sum evaluation gives other bits and does not
 * conform.)
 * Normalisation: two float32 per series, mean[s] and inv_sigma[s], set at _create (NULL: mean 0, inv_sigma 1) and by _set_stats.
 *     m_k = mean[s] 2^k;   g_k = inv_sigma[s] c_k,  c_k = (k odd ? 0x3F3504F3 : 1.0f) 2^(-floor(k/2)): the binary32 nearest 2^(-k/2)
 *     snr_k[t] = (b_k[t] - m_k) g_k           one subtraction and one multiplication, each rounded once
 * Subnormal operands or results are unspecified, as in clDedisperser.
 * Peaks: one 8-byte record {float snr; uint32 loc} per (block, series), peaks[b][r][d], loc = (k << 24) | t_in_block: the maximum of
 * snr_k[t] over k < K and the block's Tb output times.  The order is that of a 64-bit key: high word the order-preserving map of the
 * float's bits (all bits flipped if the sign bit is set, else the sign bit set), low word ~loc; the largest key wins.  So the greatest
 * S/N wins, +0 is above -0, then the smallest k, then the smallest t.  A NaN snr_k[t] never takes part; a block without a non-NaN
 * value yields {-Inf, 0xFFFFFFFF}.  +Inf inputs give +Inf peaks where the formula puts them.  A NaN at input sample t0 removes exactly
 * the snr_k[t] with t0 - 2^k < t <= t0 and nothing else.  The key maximum does not depend on the order of the reduction, so every
 * reduction shape, 64-bit integer atomicMax across workgroups included, gives the same bits.  There are no float atomics.  (While a
 * call runs, `peaks` holds its keys: the buffer is initialised, reduced into and decoded in place, all in the call's stream.)
 * Candidates (cands == NULL skips them): every peak record with snr >= threshold becomes a 16-byte record {float snr; uint32 loc;
 * uint32 series; uint32 block}, block counted from the call's first block.  threshold: _set_threshold, +Inf by default, NaN refused.
 * counts[0] = the number found, counted in full; counts[1] = the number stored = min(found, max_cands); records past the capacity are
 * dropped.  The order of the list is unspecified (an integer atomic counter, zeroed in the stream by the call).  The stored records
 * are a subset of the true set, and the whole set when found <= max_cands.
 * Invariance: either route, any split of a stream into calls at block boundaries, any legal alignment (`in` 4-byte; peaks, cands and
 * counts 8-byte) and any in_pitch give identical peak bits and an identical candidate set.
 * Routes, fixed at _create by (order, K) and named by _route():
 *   "tiled trial R=64 D=1024 K=10 Tb=1024 ns=1 w=4096 tt=3585" -- TRIAL_MAJOR, K <= 12: a workgroup stages w = 2048 (K <= 9), 4096
 *       (K <= 11) or 8192 (K = 12) samples of one series in LDS, builds the levels in place there with its own values in registers
 *       and delivers tt = w - Hs outputs;
 *   "tiled time R=64 D=1024 K=10 Tb=1024 ns=32 w=1024 tt=513" -- TIME_MAJOR, K <= 10: the same on ns = 32 series at once, whose
 *       128-byte runs per time sample are transposed into LDS rows (32 x 1025 floats and the tile's keys: 145 KiB of the 160);
 *   "generic trial R=1 D=3 K=13 Tb=16" -- TRIAL_MAJOR K = 13, TIME_MAJOR K >= 11 and every handle under _set_generic(h, 1): one thread
 *       per output walks the tree of its widest boxcar.
 * Both fused routes hold for every Tb and S.  The route is forced by _set_generic only; there is no environment switch.
 * Statistics updates: a call enqueued before _set_stats returns uses the old version entirely, a later call the new one entirely
 * (versioned device buffers; an old version is released behind the event of its last launch; nothing on the work path waits for the
 * device).  A refused update changes nothing.
 * Errors (nothing launched): NULL `in` or `peaks`, cands without counts, a misaligned buffer, `in` overlapping an output or two
 * outputs overlapping, in_pitch < n + Hs (TRIAL_MAJOR) or != 0 (TIME_MAJOR), n < 0 or n % Tb != 0, max_cands < 0, a parameter outside
 * the ranges above, a NaN threshold: MI355_ERR_INVALID_ARG.  More than 2^40 bytes per buffer and call, or 2^32 blocks and more in
 * one call: MI355_ERR_UNSUPPORTED.
 *   _plan           in_floats_per_sample = R D, history = Hs, peaks_per_block = R D; no device; any output pointer may be NULL
 *   _create         everything that can be told without a device is checked before ctx is touched; mean / inv_sigma: S floats or NULL
 *   _set_stats      replaces both arrays whole (S floats each, neither NULL);  _get_stats copies them, cap_entries is the size of each
 *   _set_threshold  the candidate threshold of every later call
 *   _history        Hs
 *   _set_generic    on != 0: the generic route for every later call of the handle; 0: back
 *   _route          valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _work           host pointers, blocking: pieces of whole blocks, each sent with its Hs samples of look-ahead; `block` of the
 *                   candidate records counts from the call's first block, as in _work_dev
 *   _work_dev       device pointers, enqueue only
 * mi355_psearch_measure: blocking and off the work path.  `in` (host, or device with in_is_device != 0) holds n >= 1 samples per
 * series in the handle's order (TRIAL_MAJOR in_pitch >= n, TIME_MAJOR 0); mean[s] and inv_sigma[s] = 1 / sqrt(population variance)
 * (host arrays of S floats) are computed on the device in float64, two passes, and rounded to float32 once; a variance of 0 gives
 * inv_sigma 0.  The values are not installed: the caller passes them to _set_stats.  The one entry that is not bit-exact.
 * ------------------------------------------------------------------------------------------------ */
#define MI355_PSEARCH_TRIAL_MAJOR 0
#define MI355_PSEARCH_TIME_MAJOR 1
typedef struct mi355_psearch mi355_psearch;
int mi355_psearch_plan(int num_rows, int num_trials, int num_widths, int block_len, int order, long long *in_floats_per_sample,
                       long long *history, long long *peaks_per_block);
int mi355_psearch_create(mi355_ctx *ctx, int num_rows, int num_trials, int num_widths, int block_len, int order, const float *mean,
                         const float *inv_sigma, mi355_psearch **out);
int mi355_psearch_destroy(mi355_psearch *h);
int mi355_psearch_set_stats(mi355_psearch *h, const float *mean, const float *inv_sigma);
int mi355_psearch_get_stats(const mi355_psearch *h, float *mean, float *inv_sigma, long long cap_entries);
int mi355_psearch_set_threshold(mi355_psearch *h, float threshold);
long long mi355_psearch_history(const mi355_psearch *h);
int mi355_psearch_set_generic(mi355_psearch *h, int on);
const char *mi355_psearch_route(const mi355_psearch *h);
int mi355_psearch_work(mi355_psearch *h, long long n, const void *in, long long in_pitch, void *peaks, void *cands, long long max_cands,
                       void *counts);
int mi355_psearch_work_dev(mi355_psearch *h, long long n, const void *in, long long in_pitch, void *peaks, void *cands, long long max_cands,
                           void *counts, void *stream);
int mi355_psearch_measure(mi355_psearch *h, long long n, const void *in, long long in_pitch, int in_is_device, float *mean, float *inv_sigma);

/* ------------------------------------------------------------------------------------------------
 * Filterbank cleaner: clFilterbankCleaner, exact RFI excision between clBeamformer's POWER output and clDedisperser: per-channel
 * normalisation over short blocks, a spectral-kurtosis channel flagger with a static channel mask, and the zero-DM filter with a
 * broadband time-sample flag.  Beyond the reference module, which has nothing of the kind (this comment is the contract).  The
 * arithmetic is pinned, so there is no tolerance anywhere.
 *     R = num_rows (beams) 1 .. 4096;  F = num_channels 1 .. 16384;  Tb = block_len, a multiple of 16 in 16 .. 4096, fixed per handle;
 *     M = (double)Tb;  L = Tb / 16.
 * Input: x[t][r][f] float32, channel fastest.  A call cleans n time samples, n a multiple of Tb; n == 0 is a no-op.  Blocks are
 * independent and the handle keeps no stream state: any split of a stream into calls at block boundaries gives identical bits.
 * Parameters, by value, changeable by _set_limits / _set_mask:
 *     nd      double > 0, finite: the raw power samples summed into one input sample times the shape factor (Ti npol for
 *             clBeamformer POWER with stokes_i)
 *     sk_lo <= sk_hi   doubles; -Inf / +Inf disable that side.  NaN is refused.
 *     td      double >= 0; +Inf disables the time-sample flag.  td2 = td td, rounded once on the host.  NaN is refused.
 *     zero_dm 0 or 1
 *     mask[f] uint8, nonzero: channel f is always flagged.  NULL at _create: all zero.
 * Step 1, statistics per (block b, r, f), IEEE binary64, x converted to double:
 *     segment s = 0 .. 15 holds the samples t = b Tb + s L .. + L - 1;
 *     a1_s = ((+0.0 + x_0) + x_1) + ...      a2_s = ((+0.0 + x_0 x_0) + x_1 x_1) + ...      in ascending t
 *     (x x is exact in double, so a fused multiply-add there gives the same bits);
 *     s1, s2 = the adjacent-pair binary tree over the 16 segment sums: (((a_0 + a_1) + (a_2 + a_3)) + ((a_4 + a_5) + (a_6 + a_7))) +
 *     (the same over a_8 .. a_15).  (A plain sequential sum gives other bits and does not conform.)
 * Step 2, the flag, every operation rounded on its own and never contracted:
 *     m = s1 / M;     var = s2 / M - m m;     sk = ((M nd + 1) / (M - 1)) ((M s2) / (s1 s1) - 1)
 *     (the generalised spectral-kurtosis estimator of Nita & Gary, 1 for clean noise);
 *     good = mask[f] == 0 && var > 0 && sk >= sk_lo && sk <= sk_hi        any NaN makes a comparison false
 *     m32 = (float)m;     is32 = (float)(1.0 / sqrt(var)), the square root IEEE correctly rounded.
 * A NaN or +-Inf anywhere in the column, or a constant column, therefore flags that (block, r, f) and reaches nothing else.
 * Step 3, normalise, binary32, two roundings: y = (x - m32) is32 for good channels, +0.0f for flagged ones.
 * Step 4, zero-DM, per (t, r), only when zero_dm is set:
 *     the binary64 partial p_j, j = 0 .. 63, starts at +0.0 and adds, in ascending f, the y of every channel with floor(f / 4) mod 64
 *     == j (flagged channels are skipped or added as +0.0: the same bits);  zs = the adjacent-pair tree over p_0 .. p_63;
 *     ng = the number of good channels of (b, r), as a double;
 *     tflag = zs zs > td2 ng;     z32 = (float)(zs / ng);
 *     y' = y - z32 for the good channels of unflagged time samples, +0.0f everywhere else (ng == 0 included).
 *   With zero_dm == 0: y' = y and every tflag is 0.
 * Outputs: out[t][r][f] float32 = y', the input's layout, directly clDedisperser's input.  Optional (NULL: not wanted):
 *     cflags[b][r][f] uint8, 1 = flagged;     tflags[t][r] uint8;
 *     stats[b][r][f] float32 pairs {m32, is32} wherever var > 0, flagged or not, and {+0.0f, +0.0f} elsewhere (8-byte aligned).
 * out == in exactly is allowed: a filterbank is cleaned in place.  Any other overlap of two buffers is MI355_ERR_INVALID_ARG.
 * Invariance: either route, any split at block boundaries, any 4-byte alignment of in / out and any n give identical bits.  There
 * are no float atomics.  Results with a subnormal float32 intermediate are unspecified, as are the bits of an output that the
 * formulas make NaN (a good channel with is32 = +Inf).
 * Routes, fixed at _create by the shape and named by _route():
 *   "slab R=64 F=1024 Tb=256 fg=256" -- F a multiple of 256 in 256 .. 4096, every Tb: ONE launch, a workgroup of 16 waves owns a
 *       (block, row) slab of Tb F floats.  Phase A: waves are segments, lanes run along channels with 16-byte loads, the segment sums
 *       of a group of fg channels meet in LDS in the contract's tree and step 2 runs once per channel.  Phase B: a wave takes a time
 *       sample, normalises, reduces its float64 partials with a cross-lane butterfly, subtracts and stores.  The slab is read twice
 *       (the second time from the caches, if they hold it) and written once.  R = 1 with few blocks per call launches few
 *       workgroups (one per block): accepted for this first form.
 *   "generic R=3 F=52 Tb=48" -- every other shape and every handle under _set_generic(h, 1): three plain kernels, one thread per
 *       (b, r, f), one per (t, r), one per output, through a scratch buffer allocated at _create (at least one block's 9 R F + 5 Tb R
 *       bytes, 16 MiB if that holds more than one); a call is walked in chunks of whole blocks that fit it.
 * The route is forced by _set_generic only; there is no environment switch.
 * Mask updates: a call enqueued before _set_mask returns uses the old mask entirely, a later call the new one entirely (versioned
 * device buffers, released behind the event of their last launch; nothing on the work path waits for the device).  A refused update,
 * of the mask or the limits, changes nothing.
 * Errors (nothing launched): NULL in or out, in or out not 4-byte aligned, stats not 8-byte aligned, overlapping buffers other than
 * out == in, n < 0 or n % Tb != 0, a parameter outside the ranges above: MI355_ERR_INVALID_ARG.  More than 2^40 bytes per buffer
 * and call: MI355_ERR_UNSUPPORTED.
 *   _plan         floats_per_sample = R F, cflag_bytes_per_block = R F, tflag_bytes_per_sample = R; no device; any pointer may be NULL
 *   _create       everything that can be told without a device is checked before ctx is touched
 *   _set_limits   by value; takes effect for the calls enqueued after it returns.  _get_limits: any pointer may be NULL
 *   _set_mask     replaces the F entries;  _get_mask copies them (as 0 / 1), cap_entries is the size of `out`
 *   _block_len    Tb
 *   _set_generic  on != 0: the generic route for every later call of the handle; 0: back
 *   _route        valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _work         host pointers, blocking: pieces of whole blocks, cleaned in place on the device
 *   _work_dev     device pointers, enqueue only: allocates nothing and waits for nothing
 * mi355_fbclean_sk_estimate (host only, no context): steps 1 and 2 on the one column x[0], x[stride], ..., x[(Tb - 1) stride]: *sk
 * receives the estimator, bit for bit what the device compares with sk_lo / sk_hi, so a caller calibrates limits without a device.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_fbclean mi355_fbclean;
int mi355_fbclean_plan(int num_rows, int num_channels, int block_len, long long *floats_per_sample, long long *cflag_bytes_per_block,
                       long long *tflag_bytes_per_sample);
int mi355_fbclean_create(mi355_ctx *ctx, int num_rows, int num_channels, int block_len, double nd, double sk_lo, double sk_hi, double td,
                         int zero_dm, const uint8_t *mask, mi355_fbclean **out);
int mi355_fbclean_destroy(mi355_fbclean *h);
int mi355_fbclean_set_limits(mi355_fbclean *h, double nd, double sk_lo, double sk_hi, double td, int zero_dm);
int mi355_fbclean_get_limits(const mi355_fbclean *h, double *nd, double *sk_lo, double *sk_hi, double *td, int *zero_dm);
int mi355_fbclean_set_mask(mi355_fbclean *h, const uint8_t *mask);
int mi355_fbclean_get_mask(const mi355_fbclean *h, uint8_t *out, long long cap_entries);
long long mi355_fbclean_block_len(const mi355_fbclean *h);
int mi355_fbclean_set_generic(mi355_fbclean *h, int on);
const char *mi355_fbclean_route(const mi355_fbclean *h);
int mi355_fbclean_work(mi355_fbclean *h, long long n, const void *in, void *out, void *cflags, void *tflags, void *stats);
int mi355_fbclean_work_dev(mi355_fbclean *h, long long n, const void *in, void *out, void *cflags, void *tflags, void *stats, void *stream);
int mi355_fbclean_sk_estimate(const float *x, int block_len, long long stride, double nd, double *sk);

/* ------------------------------------------------------------------------------------------------
 * Folder: clFolder, exact pulsar folding of the filterbank that clBeamformer POWER and clFilterbankCleaner write, modulo a known
 * period, into an archive of sub-integrations x rows x phase bins x channels.  Beyond the reference module, which has nothing of the
 * kind (this comment is the contract).  The phase is integer and the summation order is pinned, so there is no tolerance anywhere.
 *     R = num_rows (beams) 1 .. 4096;  F = num_channels 1 .. 16384;  nbin 2 .. 4096, any integer;
 *     Ts = subint_len, a multiple of 16 in 16 .. 16384, fixed per handle.
 * Input: x[t][r][f] float32, channel fastest.  Optional tflags[t][r] uint8, clFilterbankCleaner's time-flag output as it stands: a
 * nonzero flag takes that sample out of every channel of that row and out of the hit count; NULL: none.
 * Phase model, one per row: three 64-bit words {phi0, nu, nudot}.  phi0 and nu are unsigned, in 2^-64 turn and 2^-64 turn per sample;
 * nudot is signed two's complement, in 2^-64 turn per sample^2.  T is the absolute sample index of the stream, an unsigned 64-bit
 * counter kept by the handle (0 at _create; _set_sample, _skip).  All arithmetic wraps modulo 2^64, T included:
 *     tri(T) = (T even) ? (T / 2) (T - 1) : T ((T - 1) / 2)
 *     phi(T) = phi0 + nu T + nudot tri(T)
 *     bin(T) = (((phi(T) >> 32) nbin) >> 32)                      0 .. nbin - 1
 * No float touches the phase, so it does not drift at any stream length (as clFreqXlatingFIRFilter's).  Every value of the three words
 * is legal: nu = 0 puts everything of a row in one bin; periods shorter than two samples (nu >= 2^63) alias but are defined.  The
 * resolution of nudot: one unit moves the phase by 2^-64 T^2 / 2 turns, i.e. by one bin of 4096 after T = 2^26.5 ~ 9.5e7 samples; the
 * top 32 bits of the phase decide the bin, so two phases closer than 2^-32 turn may share a bin edge.
 * Stream: a call folds n samples T = T0 .. T0 + n - 1, then T0 += n.  n is a multiple of Ts; n == 0 is a no-op.  Sub-integration j of a
 * call covers its samples j Ts .. (j + 1) Ts - 1.  Sub-integrations are independent; T0 is the only stream state.
 * Outputs: out[j][r][b][f] float32, channel fastest -- a filterbank whose time axis is phase, so what reads a filterbank reads an
 * archive row.  out[j][r][b][f] starts from +0.0f and adds, in ascending T, one binary32 rounding each, every unflagged x[T][r][f] of
 * the sub-integration with bin_r(T) == b.  An empty bin is +0.0f.  Nothing is accumulated into what `out` held before.
 * Optional hits[j][r][b] uint32: the number of samples that entered (NULL: not wanted).
 * THE SUMMATION ORDER IS THE CONTRACT: a tree or a float atomic gives other bits and does not conform.  Consequences: a NaN or +-Inf
 * at (T, r, f) reaches out[j][r][bin_r(T)][f] and nothing else; a column of -0.0f folds to +0.0f.  Results with a subnormal
 * intermediate are unspecified, as elsewhere in the library.
 * Invariance: either route, any split of a stream into calls at sub-integration boundaries, _skip(n) over samples that are not folded,
 * any 4-byte alignment of in and out (hits 4-byte) and any n give identical bits.
 * Routes, fixed at _create by the shape and named by _route():
 *   "bins R=64 F=1024 nbin=256 Ts=4096" -- F a multiple of 64, every nbin and Ts.  An index launch per chunk of whole
 *       sub-integrations (1 / F of the data): a workgroup per (sub-integration, row) computes bin(T), drops the flagged samples, sorts
 *       the distinct keys (bin, t) in LDS and leaves per-bin lists, in ascending t, in a scratch buffer allocated at _create (at least
 *       one sub-integration's 4 R (Ts + nbin + 1) bytes, 16 MiB if that holds more than one); hits are the list lengths.  Then a wave
 *       owns (sub-integration, row, a group of 256, 128 or 64 channels by the largest of them that divides F, a run of bins holding
 *       about 32 rows): lanes run along channels (16-byte loads where F is a multiple of 256), the accumulators stay in registers over
 *       the bin's list, 8 rows' loads in flight before the 8 additions that consume them in order.  Bins partition time: every sample
 *       is read exactly once, there is no LDS accumulator and no float atomic, and a bin leaves as one whole channel run.
 *   "generic R=3 F=52 nbin=7 Ts=48" -- every other shape and every handle under _set_generic(h, 1): one thread per output walks its
 *       sub-integration.
 * The route is forced by _set_generic only; there is no environment switch.
 * Model updates: a call enqueued before _set_models returns uses the old table entirely, a later call the new one entirely (versioned
 * device buffers, released behind the event of their last launch; nothing on the work path waits for the device).  A refused update
 * changes nothing.
 * Errors (nothing launched, T0 unchanged): NULL in or out, in, out or hits not 4-byte aligned, any two buffers overlapping, n < 0 or
 * n % Ts != 0, a shape outside the ranges above: MI355_ERR_INVALID_ARG.  More than 2^40 bytes per buffer and call:
 * MI355_ERR_UNSUPPORTED.
 *   _plan         floats_per_sample = R F, floats_per_subint = R nbin F, hits_per_subint = R nbin; no device; any pointer may be NULL
 *   _create       models: 3 R words, row-major; everything that can be told without a device is checked before ctx is touched
 *   _set_models   replaces the 3 R words;  _get_models copies them, cap_words is the size of `out` in words
 *   _sample       *T = T0;  _set_sample: T0 = T;  _skip: T0 += n, n >= 0 (samples that are not folded)
 *   _subint_len   Ts
 *   _set_generic  on != 0: the generic route for every later call of the handle; 0: back
 *   _route        valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _work         host pointers, blocking: the shared staging pipeline in pieces of whole sub-integrations
 *   _work_dev     device pointers, enqueue only: allocates nothing and waits for nothing
 * Host-only helpers, no context:
 *   mi355_fold_model  the three words of a pulsar of period `period_s` seconds with period derivative `pdot` (s/s) sampled every
 *       `tsamp_s` seconds, at phase `phase0_turns` at T = 0, computed in long double: q = tsamp / period, nudot = -pdot q^2 (the
 *       frequency derivative -pdot / period^2 times tsamp^2), nu = q + nudot / 2 (so that nu T + nudot tri(T) is f0 t + fdot t^2 / 2 at
 *       t = T tsamp), phi0 and nu taken modulo one turn.  Rounding: each word is its long double value times 2^64 rounded to the
 *       nearest integer (ties to even), and with the errors of the long double quotient and sum each word lies within two units
 *       (2^-63) of the exact value where long double has a 64-bit significand and tsamp < period.  Refuses non-finite input, period <= 0, tsamp <= 0 and |nudot| >= 1/2.
 *   mi355_fold_bins   bins[i] = bin(T0 + i), i = 0 .. n - 1, of one model, bit for bit as the device computes it: a caller checks a
 *       setup or builds a template without a device (the counterpart of mi355_fbclean_sk_estimate).
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_fold mi355_fold;
int mi355_fold_plan(int num_rows, int num_channels, int nbin, int subint_len, long long *floats_per_sample, long long *floats_per_subint,
                    long long *hits_per_subint);
int mi355_fold_create(mi355_ctx *ctx, int num_rows, int num_channels, int nbin, int subint_len, const uint64_t *models, mi355_fold **out);
int mi355_fold_destroy(mi355_fold *h);
int mi355_fold_set_models(mi355_fold *h, const uint64_t *models);
int mi355_fold_get_models(const mi355_fold *h, uint64_t *out, long long cap_words);
int mi355_fold_sample(const mi355_fold *h, unsigned long long *T);
int mi355_fold_set_sample(mi355_fold *h, unsigned long long T);
int mi355_fold_skip(mi355_fold *h, long long n);
long long mi355_fold_subint_len(const mi355_fold *h);
int mi355_fold_set_generic(mi355_fold *h, int on);
const char *mi355_fold_route(const mi355_fold *h);
int mi355_fold_work(mi355_fold *h, long long n, const void *in, const void *tflags, void *out, void *hits);
int mi355_fold_work_dev(mi355_fold *h, long long n, const void *in, const void *tflags, void *out, void *hits, void *stream);
int mi355_fold_model(double period_s, double pdot, double tsamp_s, double phase0_turns, uint64_t out[3]);
int mi355_fold_bins(const uint64_t model[3], uint64_t T0, long long n, int nbin, int32_t *bins);

/* ------------------------------------------------------------------------------------------------
 * Period search: clPeriodSearch, an exact fast-folding search (FFA, Staelin 1969) for pulsars of unknown period over the dedispersed
 * time series that clDedisperser delivers per trial.  Its output, a period and a phase, is what mi355_fold_model takes.  Beyond the
 * reference module, which has no such block (this comment is the contract).  The arithmetic is pinned, so there is no tolerance.
 *     S = num_series 1 .. 2^20;  base periods p_lo <= p <= p_hi in samples, 16 <= p_lo <= p_hi <= 4096, P = p_hi - p_lo + 1;
 *     L = log2_rows 1 .. 12, m = 2^L;  K = num_widths 1 .. 11 with 2^(K-1) <= p_lo.
 * Input: float32, x[s in_pitch + t], t < N = m p_hi, in_pitch >= N in floats; the floats between N and in_pitch are never read.
 * Base period p uses the first m p samples of a series as m rows of p bins, row r = x[r p .. r p + p).
 * The transform, for every (s, p): a_0[r] = row r; for stage sg = 1 .. L with g = 2^sg, h = g / 2, inside every group of g consecutive
 * rows with base row B, for i < g and j < p
 *     a_sg[B + i][j] = a_(sg-1)[B + (i >> 1)][j] + a_(sg-1)[B + h + (i >> 1)][(j + ((i + 1) >> 1)) mod p]
 * each one IEEE binary32 addition, round to nearest even, the head operand on the left.  y[i] = a_L[i] is the profile of the trial
 * period p + i / (m - 1) samples: the sum over rows r of row r read at (j + sh(i, r)) mod p with
 *     sh(i, r) = sum over sg = 1 .. L of bit_(sg-1)(r) (((i >> (L - sg)) + 1) >> 1),      sh(i, m - 1) = i.
 * The tree is the contract: a left-to-right sum over rows gives other bits and does not conform.  Subnormal operands or results are
 * unspecified, as in clDedisperser.
 * Evaluation: circular dyadic boxcars per profile,
 *     b_0[j] = y[i][j];   b_k[j] = b_(k-1)[j] + b_(k-1)[(j + 2^(k-1)) mod p], k < K
 *     snr_k[j] = (b_k[j] - mean[s] 2^(L+k)) (inv_sigma[s] c_(L+k)),   c_e = (e odd ? 0x3F3504F3 : 1.0f) 2^(-floor(e/2))
 * one subtraction and one multiplication, each rounded once.  mean and inv_sigma: two float32 per series, set at _create (NULL: 0
 * and 1) and by _set_stats; the values are what mi355_psearch_measure returns.
 * peaks[s][p - p_lo][i]: one 8-byte record {float snr; uint32 loc} per trial, loc = (k << 24) | j: the maximum over k < K and j < p in
 * clPulseSearch's 64-bit key order: the greatest S/N, +0 above -0, then the smallest k, then the smallest j.  A NaN never takes
 * part; a trial without a non-NaN value gives {-Inf, 0xFFFFFFFF}.
 * profiles[s][p - p_lo][i][j] (NULL skips them): the bits of y, row pitch p_hi floats; the floats j >= p of a row are never written.
 * Invariance: either route, any partition of the stages into passes, any in_pitch, any 4-byte alignment of `in` and `profiles` and any
 * 8-byte alignment of `peaks` give identical record bits and identical profile bits wherever the formula gives no NaN; where it gives
 * a NaN the device gives a NaN (payload unspecified).  A NaN at x[r p + j0] reaches exactly the bins the formula gives for base period
 * p, and nothing of another series.
 * Routes, named by _route():
 *   "fused S=64 p=250..251 L=12 K=7 q=6,6 t=1024" -- every shape.  The stages run in passes of q stages; a workgroup of t threads
 *       gathers the 2^q rows of one independent unit into LDS, runs the q stages there and writes 2^q rows; the last pass evaluates
 *       the boxcars and reduces the keys in LDS and writes the records (and the profiles).  q is the largest with 2^q p_hi <= 32768
 *       floats, at most 8; L is split as evenly as that allows.
 *   "generic S=64 p=250..251 L=12 K=7" -- under _set_generic(h, 1): one launch per stage between two scratch planes, then one
 *       evaluation launch with a wave per trial; base periods one after another.
 * Statistics updates: a call enqueued before _set_stats returns uses the old version entirely, a later call the new one entirely
 * (versioned device buffers; nothing on the work path waits for the device).  A refused update changes nothing.
 * Errors (nothing launched): NULL `in` or `peaks`, a misaligned buffer, `in` overlapping an output or the outputs overlapping,
 * in_pitch < N, a parameter outside the ranges above: MI355_ERR_INVALID_ARG.  More than 2^40 bytes per buffer: MI355_ERR_UNSUPPORTED.
 *   _plan         N, records per series (P m), profile floats per series (P m p_hi) and the scratch bytes of a handle; no device; any
 *                 output pointer may be NULL
 *   _create       everything that can be told without a device is checked before ctx is touched; the scratch is allocated here;
 *                 mean / inv_sigma: S floats or NULL
 *   _set_stats    replaces both arrays whole (S floats each, neither NULL);  _get_stats copies them, cap_entries is the size of each
 *   _set_generic  on != 0: the generic route for every later call of the handle; 0: back
 *   _route        valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _work         host pointers, blocking: pieces of whole series through device scratch of the handle
 *   _work_dev     device pointers, enqueue only: allocates nothing and waits for nothing
 * Host-only helpers, no context:
 *   mi355_ffa_shift   sh(i, r) for i, r < 2^log2_rows; MI355_ERR_INVALID_ARG (negative) outside the ranges
 *   mi355_ffa_period  (p + i / (2^log2_rows - 1)) tsamp_s in double seconds, the argument of mi355_fold_model; NaN outside the ranges
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_ffa mi355_ffa;
int mi355_ffa_plan(int num_series, int p_lo, int p_hi, int log2_rows, int num_widths, long long *in_floats_per_series,
                   long long *records_per_series, long long *profile_floats_per_series, long long *scratch_bytes);
int mi355_ffa_create(mi355_ctx *ctx, int num_series, int p_lo, int p_hi, int log2_rows, int num_widths, const float *mean,
                     const float *inv_sigma, mi355_ffa **out);
int mi355_ffa_destroy(mi355_ffa *h);
int mi355_ffa_set_stats(mi355_ffa *h, const float *mean, const float *inv_sigma);
int mi355_ffa_get_stats(const mi355_ffa *h, float *mean, float *inv_sigma, long long cap_entries);
int mi355_ffa_set_generic(mi355_ffa *h, int on);
const char *mi355_ffa_route(const mi355_ffa *h);
int mi355_ffa_work(mi355_ffa *h, const void *in, long long in_pitch, void *peaks, void *profiles);
int mi355_ffa_work_dev(mi355_ffa *h, const void *in, long long in_pitch, void *peaks, void *profiles, void *stream);
long long mi355_ffa_shift(int log2_rows, int i, int r);
double mi355_ffa_period(int p, int log2_rows, int i, double tsamp_s);

/* ------------------------------------------------------------------------------------------------
 * Spectral search: clSpectralSearch, the Fourier-domain periodicity search over the dedispersed time series that clDedisperser delivers
 * per trial: transform, normalised power spectrum, incoherent harmonic sums of 1, 2, 4 .. 32 harmonics, peaks.  The one step that sees
 * periods below clPeriodSearch's 16 samples, O(N log N) per series.  Beyond the reference module, which has no such block (this
 * comment is the contract).  Two stages: the spectrum is floating point and held to a derived bound against float64
 * (tests/ssearch_ref.py); the harmonic sums are pinned arithmetic, compared bit for bit.
 *     S = num_series 1 .. 2^20;  N = n, a power of two 2^8 .. 2^22 samples per series, Nb = N / 2 bins;  H = num_folds 0 .. 5 (level h
 *     sums 2^h harmonics);  Bb = block_bins, a power of two 16 .. Nb;  k_lo 1 .. Nb - 1;  input_kind SERIES (0) or SPECTRUM (1).
 * Spectrum stage (SERIES input): x[s in_pitch + t] float32, t < N, in_pitch >= N and even, `in` 8-byte aligned; the floats between N and
 * in_pitch are never read.  The series is read as Nb complex items z[n] = x[2n] + i x[2n+1] and transformed by an internal clFFT handle
 * of Nb points (no copy when in_pitch == N and the transform can take the input as it lies; otherwise rows of N floats are packed
 * through scratch first -- a frame of clFFT depends on its own input alone, so the bits are the same).  One kernel untangles and detects:
 *     X[k] = (Z[k] + conj Z[Nb-k]) / 2 - i e^(-2 pi i k / N) (Z[k] - conj Z[Nb-k]) / 2,   0 <= k < Nb,  Z[Nb] = Z[0]
 *     w[s][k] = (Re X^2 + Im X^2) g[s],  g[s] = inv_sigma[s]^2 / N;   w[s][k] = +0 for k < k_lo;   the Nyquist bin is dropped
 * with twiddles rounded once from double (exact 0 and 1 at the ends).  White noise of variance sigma^2 gives w a mean of 1.
 * inv_sigma: one float32 per series, what mi355_psearch_measure returns, set at _create (NULL: 1) and by _set_stats; no mean is needed
 * (it lands in bin 0, below k_lo).  `spectrum` (NULL skips it): spectrum[s Nb + k] holds the bits of w.  The bits of w do not depend on
 * in_pitch, on the alignment, on which other series share the call or on a split of the series into calls.
 * Harmonic-sum stage (SPECTRUM input runs it on w[s in_pitch + k] from `in` directly, in_pitch >= Nb, 4-byte aligned): with the integer
 * index r(k, j, h) = (k j + 2^(h-1)) >> h, which is never above k,
 *     s_0[k] = w[k]
 *     s_h[k] = (...((s_(h-1)[k] + w[r(k,1,h)]) + w[r(k,3,h)]) + ...) + w[r(k,2^h-1,h)]                 h = 1 .. H
 *     snr_h[k] = (s_h[k] - 2^h) c_h,   c_h = (h odd ? 0x3F3504F3 : 1.0f) 2^(-floor(h/2))   (clPulseSearch's constant)
 * every + one binary32 addition, round to nearest even, the accumulator on the left, odd j ascending, level after level; the S/N one
 * subtraction and one multiplication, each rounded once.  Bin k of level h is the 2^h-th harmonic: the fundamental is k / 2^h bins.
 * The order is the contract: descending j, or summing a level first and adding it after, gives other bits and does not conform.
 * Subnormal operands or results are unspecified, as in clDedisperser.
 * Peaks: one 8-byte record {float snr; uint32 loc} per (series, block), peaks[s][b], b < Nb / Bb, loc = (h << 24) | k_in_block: the
 * maximum over h <= H and the block's Bb bins in clPulseSearch's 64-bit key order -- the greatest S/N, +0 above -0, then the smallest h,
 * then the smallest k.  A NaN never takes part; a block without a non-NaN value gives {-Inf, 0xFFFFFFFF}.  A NaN at w[m] removes exactly
 * the (h, k) whose sum reads m, and nothing of another series.  The key maximum does not depend on the order of the reduction, so
 * 64-bit integer atomicMax across workgroups gives the same bits; there are no float atomics.  (While a call runs, `peaks` holds its
 * keys: initialised, reduced into and decoded in place, all in the call's stream.)
 * Candidates (cands == NULL skips them), as clPulseSearch: every record with snr >= threshold becomes {float snr; uint32 loc; uint32
 * series; uint32 block}; _set_threshold, +Inf by default, NaN refused; counts[0] = found, counted in full, counts[1] = stored =
 * min(found, max_cands); the order of the list is unspecified (an integer counter, zeroed in the stream by the call).
 * Invariance: either route, any in_pitch, any legal alignment and any split of the series into calls give identical peak bits, an
 * identical candidate set and identical spectrum bits.
 * Routes, named by _route() and forced by _set_generic only (no environment switch):
 *   "tiled S=2 N=16384 H=5 Bb=256 tk=1024 ..." -- the default: a workgroup owns (series, tile of tk = min(Nb, 1024) bins), stages per
 *       level the contiguous window of every odd j in LDS (at most 8 tk + 128 floats at h = 5, 33 KiB), a thread keeps the running sums
 *       of its four bins in registers across the levels; keys by DPP, LDS and one 64-bit atomicMax per (tile, block);
 *   "generic S=2 N=16384 H=5 Bb=256 ..." -- under _set_generic(h, 1): one thread per bin gathers from global memory.
 *   The tail names the input: "spectrum", or "series k_lo=.. chunk=.. fft=.." (series per chunk of the spectrum stage, the length of
 *   the internal transform) and the packing policy: rows are packed through scratch when in_pitch != N, or when the transform has more
 *   than 4096 points and `in` is not 16-byte aligned.
 * Statistics updates: a call enqueued before _set_stats returns uses the old version entirely, a later call the new one entirely.
 * Errors (nothing launched): NULL `in` or `peaks`, cands without counts, a misaligned buffer (`in` 8-byte with SERIES and 4-byte with
 * SPECTRUM input, spectrum 4-byte, peaks, cands and counts 8-byte), `in` overlapping an output or two outputs overlapping, in_pitch too
 * small or, with SERIES input, odd, max_cands < 0, a parameter outside the ranges above, a NaN threshold, a `spectrum` output with
 * SPECTRUM input: MI355_ERR_INVALID_ARG.  More than 2^40 bytes per buffer: MI355_ERR_UNSUPPORTED.
 *   _plan           spectrum floats per series (Nb), records per series (Nb / Bb) and the scratch bytes of a handle (SERIES: a chunk's
 *                   packed input, Z and w; SPECTRUM: 0); no device; any output pointer may be NULL
 *   _create         everything that can be told without a device is checked before ctx is touched; the scratch is allocated here and
 *                   the internal transform has run once on a chunk of zeros, so its workspace exists; inv_sigma: S floats or NULL
 *   _set_stats      replaces the array whole (S floats);  _get_stats copies it, cap_entries is its size
 *   _set_threshold  the candidate threshold of every later call
 *   _set_generic    on != 0: the generic route for every later call of the handle; 0: back
 *   _route          valid until the next _set_generic / _destroy of the handle; "" for NULL
 *   _fft_route      mi355_fft_last_route of the internal transform's last call, which selects the multiple of the spectrum bound; ""
 *                   for NULL, with SPECTRUM input and before the first call.  Valid until the handle's next _work / _work_dev /
 *                   _destroy; read without the handle's lock, so a caller that works on the handle from another thread at the
 *                   same time gets either call's route
 *   _work           host pointers, blocking: pieces of whole series through device scratch of the handle
 *   _work_dev       device pointers, enqueue only: allocates nothing and waits for nothing
 * Host-only helper, no context:
 *   mi355_ssearch_freq  the fundamental k / (2^h N tsamp_s) in Hz of bin k of level h, as a double; its reciprocal is the period
 *                       mi355_fold_model takes; NaN outside the ranges (N as above, tsamp_s > 0 and finite, h 0 .. 5, k 0 .. Nb - 1)
 * ------------------------------------------------------------------------------------------------ */
#define MI355_SSEARCH_SERIES 0
#define MI355_SSEARCH_SPECTRUM 1
typedef struct mi355_ssearch mi355_ssearch;
int mi355_ssearch_plan(int num_series, int n, int num_folds, int block_bins, int k_lo, int input_kind, long long *spectrum_floats_per_series,
                       long long *records_per_series, long long *scratch_bytes);
int mi355_ssearch_create(mi355_ctx *ctx, int num_series, int n, int num_folds, int block_bins, int k_lo, int input_kind, const float *inv_sigma,
                         mi355_ssearch **out);
int mi355_ssearch_destroy(mi355_ssearch *h);
int mi355_ssearch_set_stats(mi355_ssearch *h, const float *inv_sigma);
int mi355_ssearch_get_stats(const mi355_ssearch *h, float *inv_sigma, long long cap_entries);
int mi355_ssearch_set_threshold(mi355_ssearch *h, float threshold);
int mi355_ssearch_set_generic(mi355_ssearch *h, int on);
const char *mi355_ssearch_route(const mi355_ssearch *h);
const char *mi355_ssearch_fft_route(const mi355_ssearch *h);
int mi355_ssearch_work(mi355_ssearch *h, const void *in, long long in_pitch, void *peaks, void *spectrum, void *cands, long long max_cands,
                       void *counts);
int mi355_ssearch_work_dev(mi355_ssearch *h, const void *in, long long in_pitch, void *peaks, void *spectrum, void *cands, long long max_cands,
                           void *counts, void *stream);
double mi355_ssearch_freq(int n, double tsamp_s, int h, int k);

/* ------------------------------------------------------------------------------------------------
 * Acceleration trials: clAccelResampler, the time-domain resampling step that deployed acceleration searches (peasoup, SIGPROC's seek)
 * run between dedispersion and the period search: every dedispersed series is stretched quadratically once per acceleration trial, and
 * the unchanged clSpectralSearch (the S A output rows are its series as they lie), clPeriodSearch and mi355_psearch_measure run on every
 * copy.  A pulsar in a binary drifts across spectral bins at constant period; at the right trial its peak is whole again.  Beyond the
 * reference module, which has no such block (this comment is the contract).  A pure gather with an integer index: the block moves
 * 32-bit words and does no arithmetic on them, so NaN payloads, -0 and subnormals arrive unchanged, and every output word is pinned.
 *     S = num_series 1 .. 2^20;  N = n 256 .. 2^22, any integer;  A = num_trials 1 .. 4096;  one signed 64-bit coefficient c[a] per
 *     trial in units of 2^-64 sample per sample^2, with |c[a]| N <= 2^63.
 * The index map, in exact integers (a signed 128-bit product, floor division, so a tie rounds up):
 *     d(i)     = i (N - i)
 *     delta_a(i) = floor((c[a] d(i) + 2^63) / 2^64)
 *     src_a(i) = i + delta_a(i)                                                        0 <= i < N
 *     out[((s na) + (a - a0)) out_pitch + i] = in[s in_pitch + src_a(i)]               0 <= s < S,  a0 <= a < a0 + na
 * No float touches the index: truncation toward zero instead of the floor, or an index computed in float64, is another function and
 * does not conform.  For the ranges above (tests/test_accel.py proves them with Python integers): src_a(0) = 0, src_a(N-1) = N-1,
 * src_a is non-decreasing in i (and, d being non-negative, in c), |delta_a(i)| <= N / 8 (reached at c = +-2^63 / N), and c = 0 is the
 * identity.  So every source lies inside its own series and nothing outside it is read.
 * A call takes the trial range [a0, a0 + na): a caller walks a ladder whose whole output would not fit in memory.  The output rows of
 * a call are S na series of N samples at out_pitch, series-major, then trial.
 * Buffers: `in` and `out` 4-byte aligned, both pitches at least N; the words between N and a pitch are neither read nor written.
 * Invariance: either route, any split over series or trial ranges into calls, any legal in_pitch, out_pitch and alignment give
 * identical bits.
 * Routes, named by _route() and forced by _set_generic only (no environment switch):
 *   "tiled S=64 N=1048576 A=16 tile=1024 group=16" -- the default at every shape: a workgroup owns (series, tile of 1024 outputs,
 *       group of consecutive trials), stages the union of the group's source windows in LDS once (16-byte loads of whole aligned
 *       pieces), and a wave writes one trial's tile at a time: a lane owns runs of four outputs that start at a 16-byte boundary of
 *       `out` and leave as one 16-byte store; a trial's tiles meet on those boundaries, so only what lies in front of a row's first
 *       boundary and behind its last leaves as 4-byte stores.
 *       The index is carried along a run by its first and second differences in 128 bits and the shift is taken at every sample
 *       (d is concave: equal shifts at the two ends of a run do not make it constant inside).  The series is read once per group.
 *       group = the largest g <= 16 at which every run of g consecutive trials of the table fits the LDS budget of 4096 words: a
 *       window holds at most 1544 + ceil((cmax - cmin) N^2 / 2^66) words (the map's slope is below 3/2, so one trial always fits; the
 *       second term is the spread of the group's shifts at mid-series).  Recomputed by _set_trials; an unsorted, widely spread table
 *       gives group = 1.
 *   "generic S=64 N=1048576 A=16" -- under _set_generic(h, 1): one thread per output gathers from global memory.
 *   Measured on an MI355X (tools/accel_probe.py, README.md): where a group shares its window (A >= 4) the tiled route takes 0.40 - 0.47x
 *   the generic route's time; with a single trial the two tie (the generic route 1.5 % ahead at S = 1024, N = 2^20).  The tiled route is
 *   the default at every shape.
 * Trial updates: the table is a versioned device buffer, released behind its last launch's event; a call enqueued before _set_trials
 * returns uses the old table (and its group size) entirely, a later call the new one entirely.
 * Errors (nothing launched): NULL `in` or `out`, a misaligned buffer, `in` overlapping `out`, a trial range outside 0 .. A or empty,
 * a pitch below N, a parameter outside the ranges above, a coefficient outside the bound: MI355_ERR_INVALID_ARG.  More than 2^40 bytes
 * per buffer: MI355_ERR_UNSUPPORTED.
 *   _plan        output rows of the whole ladder (S A), the tile and the bytes of the device table; no device; any output pointer
 *                may be NULL
 *   _create      everything that can be told without a device is checked before ctx is touched; c: A coefficients, NULL = all 0
 *   _set_trials  replaces the table whole (A coefficients);  _get_trials copies it, cap_entries is its size
 *   _set_generic on != 0: the generic route for every later call of the handle; 0: back
 *   _route       valid until the next _set_trials / _set_generic / _destroy of the handle; "" for NULL
 *   _work        host pointers, blocking: pieces of whole series, and per piece runs of whole trials, through device scratch of the
 *                handle
 *   _work_dev    device pointers, enqueue only: allocates nothing and waits for nothing
 * Host-only helpers, no context:
 *   mi355_accel_coeff   c = round(-2^64 accel tsamp / (2 x 299792458)) of a line-of-sight acceleration in m/s^2, computed in long double:
 *                       within two units of the exact rational value of the double inputs; a result outside the bound, n outside its
 *                       range, tsamp_s not positive and finite or accel not finite: MI355_ERR_INVALID_ARG (c = 0 then)
 *   mi355_accel_index   src(i) for i0 <= i < i0 + count, the map on the host bit for bit
 *   mi355_accel_trials  the ladder a_j = j da for the integers j with a_lo <= a_j <= a_hi, ascending, da = tol 8 x 299792458 /
 *                       (tsamp N^2): neighbouring trials differ by tol samples at mid-observation; j = 0 gives c = 0 exactly, the
 *                       identity.  count is always the full count of the ladder (it may be 0 and may exceed 4096); at most cap
 *                       coefficients are stored.  A trial outside the bound is an error whatever cap is.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mi355_accel mi355_accel;
int mi355_accel_plan(int num_series, int n, int num_trials, long long *rows, long long *tile, long long *table_bytes);
int mi355_accel_create(mi355_ctx *ctx, int num_series, int n, int num_trials, const long long *c, mi355_accel **out);
int mi355_accel_destroy(mi355_accel *h);
int mi355_accel_set_trials(mi355_accel *h, const long long *c);
int mi355_accel_get_trials(const mi355_accel *h, long long *c, long long cap_entries);
int mi355_accel_set_generic(mi355_accel *h, int on);
const char *mi355_accel_route(const mi355_accel *h);
int mi355_accel_work(mi355_accel *h, const void *in, long long in_pitch, void *out, long long out_pitch, int a0, int na);
int mi355_accel_work_dev(mi355_accel *h, const void *in, long long in_pitch, void *out, long long out_pitch, int a0, int na, void *stream);
int mi355_accel_coeff(int n, double tsamp_s, double accel_m_s2, long long *c);
int mi355_accel_index(int n, long long c, long long i0, long long count, long long *src);
int mi355_accel_trials(int n, double tsamp_s, double a_lo, double a_hi, double tol_samples, long long *c, long long cap, long long *count);

#ifdef __cplusplus
}
#endif
#endif /* MI355_CLENABLED_H */
