// Every public header of the MI355X build of gr::clenabled in one include (the block layer, the CLI and the pybind module use
// this; users of the reference keep including <clenabled/clFFT.h>, <clenabled/clFilter.h>, ... one per block, exactly as
// before: the reference installs include/clenabled/<Block>.h, and so does this build -- tests/test_host_cpp.py compiles a
// translation unit per header).
#pragma once
#include "GRCLBase.h"
#include "clMathOpTypes.h"
#include "clSComplex.h"
#include "clMathOp.h"
#include "clMathConst.h"
#include "clFFT.h"
#include "clFilter.h"
#include "clComplexFilter.h"
#include "clPolyphaseChannelizer.h"
#include "clXEngine.h"
// widened rows
#include "clLog.h"
#include "clSNR.h"
#include "clComplexToMag.h"
#include "clComplexToArg.h"
#include "clComplexToMagPhase.h"
#include "clMagPhaseToComplex.h"
#include "clQuadratureDemod.h"
#include "clxcorrelate_fft_vcf.h"

#include <limits>

namespace gr {
namespace clenabled {

// gr::clenabled::clXCorrelate -- make() as the reference's include/clenabled/clXCorrelate.h:55-56.  Time-domain lag search of
// inputs 1..num_inputs-1 against input 0 over frames of signal_length items (data_size bytes each: complex 8 / float 4); no
// outputs, one message port "corr" carrying {"corrvect": f32vector, "corrective_lags": s32vector} per processed frame
// (lib/clXCorrelate_impl.cc:1594-1600).  (The reference's per-block header of this name is not installed by this build yet.)
class CLENABLED_API clXCorrelate : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clXCorrelate> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, bool setDebug, int num_inputs,
                     int signal_length, int data_type, int data_size, int max_search_index, int decim_frames, bool async = false);
    // the effective max shift (max_search_index rounded up to a power of two, :716-747)
    virtual int max_shift() const = 0;
    virtual int signal_length() const = 0;  // items per frame (the output multiple)
    // async: block until the running submission (if any) has finished; its result is published with the next accepted frame
    virtual void wait() = 0;
};

// gr::clenabled::clSignalSource -- make() as the reference's include/clenabled/clSignalSource.h:49-50.  NCO / tone generator: no
// inputs, one output of complex, float or int items; waveform 1 cos, 2 sin (complex items carry both).  The phase advances from
// call to call and set_frequency() keeps it.  (The reference's per-block header of this name is not installed by this build yet.)
class CLENABLED_API clSignalSource : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clSignalSource> sptr;
    static sptr make(int idataType, int openCLPlatformType, int devSelector, int platformId, int devId, double samp_rate, int waveform,
                     double freq, float amplitude, int setDebug = 0);
    virtual void set_frequency(double frequency) = 0;  // lib/clSignalSource_impl.cc:251
    virtual void set_phase(double angle_pos) = 0;
    virtual double get_angle_pos() const = 0;   // phase of the next call's first item, radians
    virtual double get_angle_rate() const = 0;  // 2 pi freq / samp_rate
};

// gr::clenabled::clCostasLoop -- make() as the reference's include/clenabled/clCostasLoop.h:52; order 2 (BPSK) or 4 (QPSK), anything
// else throws std::invalid_argument (lib/clCostasLoop_impl.cc:80-83).  One complex input; output 0 the de-rotated stream, the
// optional output 1 the loop frequency per item (float).  The reference inherits gr::blocks::control_loop; this class carries the
// part of that interface a flowgraph uses itself.  (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clCostasLoop : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clCostasLoop> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, float loop_bw, int order, int setDebug = 0);
    virtual void set_loop_bandwidth(float bw) = 0;
    virtual float get_loop_bandwidth() const = 0;
    virtual float get_alpha() const = 0;
    virtual float get_beta() const = 0;
    virtual float get_frequency() const = 0;  // these two wait for the block's last work() call
    virtual float get_phase() const = 0;
    virtual void set_frequency(float freq) = 0;
    virtual void set_phase(float phase) = 0;
};

// gr::clenabled::clRationalResampler -- polyphase FIR with interpolation L and decimation M, the contract of GNU Radio's
// rational_resampler_ccf (make) / _ccc (make_ccc); decimation 1 is interp_fir_filter.  Beyond the reference module.  A general
// block: history ceil(ntaps / L), relative rate L / M, output multiple 1; L and M are used as given (not reduced by their gcd)
// and the taps carry the gain L.  taps() reports real taps with a zero imaginary part; set_taps() keeps the resampling phase.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clRationalResampler : virtual public gr::block {
public:
    typedef std::shared_ptr<clRationalResampler> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int interpolation, int decimation,
                     const std::vector<float> &taps, int setDebug = 0);
    static sptr make_ccc(int openCLPlatformType, int devSelector, int platformId, int devId, int interpolation, int decimation,
                         const std::vector<gr_complex> &taps, int setDebug = 0);
    virtual std::vector<gr_complex> taps() const = 0;
    virtual void set_taps(const std::vector<gr_complex> &taps) = 0;  // a block made with real taps refuses a non-zero imaginary part
    virtual int interpolation() const = 0;
    virtual int decimation() const = 0;
};

// gr::clenabled::clPolyphaseSynthesizer -- critically sampled inverse-DFT polyphase synthesis bank, the counterpart of
// clPolyphaseChannelizer: the input stream is that block's item-major multiplex (frames of nmap = ch_map.size() items, slot q
// feeding channel ch_map[q]; an empty ch_map: all num_channels channels in order), the output the wideband stream.  Beyond the
// reference module; the contract is in mi355_clenabled.h.  A general block: history (taps_per_arm - 1) nmap + 1, relative rate
// num_channels / nmap, output multiple num_channels; it consumes whole frames only and the taps carry the gain.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clPolyphaseSynthesizer : virtual public gr::block {
public:
    typedef std::shared_ptr<clPolyphaseSynthesizer> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, const std::vector<float> &taps, int num_channels,
                     const std::vector<int> &ch_map = std::vector<int>(), int setDebug = 0);
    virtual std::vector<float> taps() const = 0;
    virtual void set_taps(const std::vector<float> &taps) = 0;  // may change taps_per_arm, and with it the history
    virtual int taps_per_arm() const = 0;
    virtual int num_channels() const = 0;
    virtual int nmap() const = 0;
    virtual std::string route() const = 0;
};

// gr::clenabled::clPowerSpectrum -- window, forward DFT, |X|^2, mean over navg frames that start hop items apart (0: fft_size), optionally
// fftshift and 10 log10: the spectrum estimator (logpwrfft, Bartlett / Welch periodogram) in one block.  Beyond the reference module; the
// contract is in mi355_clenabled.h.  A general block from complex items to vectors of fft_size floats: history max(fft_size - hop, 0) + 1,
// one output vector per navg * hop items consumed (with hop > fft_size a spectrum is made once all navg * hop items are offered: the
// block never consumes more than that).  An empty window is all ones.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clPowerSpectrum : virtual public gr::block {
public:
    typedef std::shared_ptr<clPowerSpectrum> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int fft_size, int navg,
                     const std::vector<float> &window = std::vector<float>(), int hop = 0, bool shift = false, bool log_output = false,
                     float scale = 1.0f, int setDebug = 0);
    virtual int fft_size() const = 0;
    virtual int navg() const = 0;
    virtual int hop() const = 0;
    virtual void set_scale(float scale) = 0;
    virtual void set_window(const std::vector<float> &window) = 0;  // empty: all ones
    virtual void set_generic(bool on) = 0;                          // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clFreqXlatingFIRFilter -- tune + FIR + decimate, the contract of GNU Radio's freq_xlating_fir_filter_ccf (make) / _ccc
// (make_ccc), for one or several centre frequencies at once: one complex input, one complex output stream per centre frequency, all
// formed from one read of the input.  Beyond the reference module; the contract is in mi355_clenabled.h.  A sync_decimator with
// history ntaps; the message port "freq" retunes channel 0 (a pair whose cdr is a real number, as GNU Radio's block takes it).  The phase
// of every channel is a 64-bit integer and stays continuous across set_center_freq(); taps() reports real taps with a zero imaginary
// part.  set_taps() takes effect at once; the work() call after it only installs the new history and produces nothing (clFilter's rule).
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clFreqXlatingFIRFilter : virtual public gr::sync_decimator {
public:
    typedef std::shared_ptr<clFreqXlatingFIRFilter> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int decimation, const std::vector<float> &taps,
                     const std::vector<double> &center_freqs, double sampling_freq, bool use_time = false, int setDebug = 0);
    static sptr make_ccc(int openCLPlatformType, int devSelector, int platformId, int devId, int decimation, const std::vector<gr_complex> &taps,
                         const std::vector<double> &center_freqs, double sampling_freq, bool use_time = false, int setDebug = 0);
    virtual void set_center_freq(double center_freq, int channel = 0) = 0;
    virtual double center_freq(int channel = 0) const = 0;
    virtual std::vector<gr_complex> taps() const = 0;
    virtual void set_taps(const std::vector<gr_complex> &taps) = 0;  // a block made with real taps refuses a non-zero imaginary part
    virtual int num_channels() const = 0;
    virtual void skip(long long noutputs) = 0;  // advance every phase as if that many outputs had been made (dropped upstream samples)
    virtual void set_generic(bool on) = 0;      // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clBeamformer -- tied-array beamformer on the X-engine's int8 frames: num_beams weighted sums of the num_inputs stations
// per channel and polarisation, complex int8 weights, integer-exact.  Beyond the reference module; the contract is in mi355_clenabled.h.
// One input stream whose item is a frame (frame_bytes() = 2 num_inputs num_channels npol bytes), one output stream whose item is a unit's
// output: mode 0 (VOLTAGE) num_beams num_channels npol gr_complex per frame -- decimation 1, a sync_block in all but name -- and mode 1
// (POWER) num_beams num_channels (stokes_i ? 1 : npol) floats per `integration` frames, a sync_decimator by `integration`.  Weights are
// int8 {re, im} in the layout [f][p][b][s], -127 .. 127; an empty vector at make() is all zero.  There is no message port: weights are
// set through set_weights() / set_beam_weights(), and a work() call uses one weight set entirely.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clBeamformer : virtual public gr::sync_decimator {
public:
    typedef std::shared_ptr<clBeamformer> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int mode, int polarization, int num_inputs,
                     int num_channels, int num_beams, int integration = 1, bool stokes_i = false,
                     const std::vector<int8_t> &weights = std::vector<int8_t>(), int setDebug = 0);
    virtual void set_weights(const std::vector<int8_t> &weights) = 0;                     // 2 F npol B S bytes, anything else throws
    virtual void set_beam_weights(int beam, const std::vector<int8_t> &w_beam) = 0;      // 2 F npol S bytes, [f][p][s]
    virtual std::vector<int8_t> weights() const = 0;
    virtual int num_beams() const = 0;
    virtual long long frame_bytes() const = 0;
    virtual long long out_bytes_per_unit() const = 0;
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clFEngine -- the F-engine in front of clXEngine and clBeamformer: num_inputs stations of `polarization` complex streams
// (input r = s npol + p) through a critically sampled polyphase filter bank (taps: taps_per_channel * num_channels real prototype taps,
// empty = all ones), a forward DFT, a real gain per (input, channel) and symmetric int8 quantisation into the frames
// [t][station][chan][pol]{I, Q}.  Beyond the reference module; the contract is in mi355_clenabled.h.  A sync_decimator over R = S npol
// gr_complex inputs with decimation num_channels and history (taps_per_channel - 1) num_channels + 1; its one output item is a frame of
// frame_bytes() = 2 S num_channels npol bytes, the item clBeamformer takes in.  gains: R num_channels floats, [r][f]; empty = all 1.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clFEngine : virtual public gr::sync_decimator {
public:
    typedef std::shared_ptr<clFEngine> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int polarization, int num_inputs, int num_channels,
                     const std::vector<float> &taps = std::vector<float>(), int taps_per_channel = 1, bool shift = false,
                     const std::vector<float> &gains = std::vector<float>(), int setDebug = 0);
    virtual void set_gains(const std::vector<float> &gains) = 0;                  // R num_channels floats, anything else throws
    virtual void set_input_gain(int input, const std::vector<float> &gain) = 0;   // num_channels floats
    virtual std::vector<float> gains() const = 0;
    virtual std::vector<uint64_t> clips(bool reset = false) = 0;                  // saturated or NaN components per input (waits for the device)
    virtual long long frame_bytes() const = 0;
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clDedisperser -- exact incoherent dedispersion behind clBeamformer's POWER output: num_rows x num_channels floats per time
// sample summed over the channels at per-(trial, channel) sample delays, in ascending channel order with one binary32 rounding per
// addition.  Beyond the reference module; the contract is in mi355_clenabled.h.  A sync_block: one input stream whose item is a time
// sample of num_rows num_channels floats ([row][chan], the item clBeamformer writes in POWER mode with stokes_i or one polarisation),
// one output stream whose item is num_rows num_trials floats ([row][trial], TIME_MAJOR), history max_delay + 1.  delays: int32
// [trial][chan], each 0 .. max_delay or -1 (the channel takes no part in the trial); an empty vector at make() is all zero.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clDedisperser : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clDedisperser> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels, int num_trials,
                     int max_delay, const std::vector<int32_t> &delays = std::vector<int32_t>(), int setDebug = 0);
    virtual void set_delays(const std::vector<int32_t> &delays) = 0;  // num_trials num_channels entries, anything else throws
    virtual std::vector<int32_t> delays() const = 0;
    virtual int max_delay() const = 0;
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;  // may change with set_delays()
};

// gr::clenabled::clPulseSearch -- exact boxcar single-pulse search behind clDedisperser: per series num_widths boxcars of widths
// 2^0 .. 2^(num_widths - 1) summed as a fixed dyadic tree of binary32 additions, normalised to S/N with a mean and an inverse sigma per
// series, reduced to one peak per (block of block_len samples, series).  Beyond the reference module; the contract is in
// mi355_clenabled.h.  A sync_decimator by block_len: one input stream whose item is a time sample of num_rows num_trials floats
// ([row][trial], the item clDedisperser writes), one output stream whose item is num_rows num_trials peak records of 8 bytes
// ({float snr; uint32 loc = (k << 24) | t_in_block}), history 2^(num_widths - 1).  mean / inv_sigma: num_rows num_trials floats each;
// empty vectors at make() are mean 0 and inv_sigma 1.  Candidates are not exposed at this layer (no message port).
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clPulseSearch : virtual public gr::sync_decimator {
public:
    typedef std::shared_ptr<clPulseSearch> sptr;
    struct peak {
        float snr;
        uint32_t loc;
    };
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_trials, int num_widths,
                     int block_len, const std::vector<float> &mean = std::vector<float>(), const std::vector<float> &inv_sigma = std::vector<float>(),
                     int setDebug = 0);
    virtual void set_stats(const std::vector<float> &mean, const std::vector<float> &inv_sigma) = 0;  // num_rows num_trials entries each, anything else throws
    virtual std::vector<float> mean() const = 0;
    virtual std::vector<float> inv_sigma() const = 0;
    virtual int lookahead() const = 0;      // 2^(num_widths - 1) - 1
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clFilterbankCleaner -- exact RFI excision between clBeamformer's POWER output and clDedisperser: per (block of block_len
// samples, row, channel) float64 statistics in a pinned order, a channel flag (static mask, variance > 0, sk_lo <= spectral kurtosis <=
// sk_hi), normalisation to zero mean and unit variance, and with zero_dm the mean over the good channels removed per time sample, time
// samples whose sum exceeds td sigma zeroed.  Beyond the reference module; the contract is in mi355_clenabled.h.  A sync_block with
// output multiple block_len and no history: one input stream whose item is a time sample of num_rows num_channels floats ([row][chan],
// the item clBeamformer writes in POWER mode), output 0 the same item cleaned (the item clDedisperser reads); the optional output 1
// carries num_rows time-sample flag bytes per item, the optional output 2 the num_rows num_channels channel-flag bytes of the block
// the item lies in (repeated for every item of the block).  mask: num_channels bytes, nonzero = always flagged; empty = none.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clFilterbankCleaner : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clFilterbankCleaner> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels, int block_len,
                     double nd = 1.0, double sk_lo = -std::numeric_limits<double>::infinity(), double sk_hi = std::numeric_limits<double>::infinity(),
                     double td = std::numeric_limits<double>::infinity(), bool zero_dm = false,
                     const std::vector<uint8_t> &mask = std::vector<uint8_t>(), int setDebug = 0);
    virtual void set_limits(double nd, double sk_lo, double sk_hi, double td, bool zero_dm) = 0;  // for the calls after it returns
    virtual std::vector<double> limits() const = 0;                                               // {nd, sk_lo, sk_hi, td, zero_dm}
    virtual void set_mask(const std::vector<uint8_t> &mask) = 0;                                  // num_channels entries, anything else throws
    virtual std::vector<uint8_t> mask() const = 0;
    virtual int block_len() const = 0;
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clFolder -- exact pulsar folding of the filterbank that clBeamformer POWER and clFilterbankCleaner write, modulo a
// known period: an integer phase model {phi0, nu, nudot} per row (units of 2^-64 turn; mi355_fold_model makes one), sums per (row,
// phase bin, channel) in ascending time with one binary32 rounding each.  Beyond the reference module; the contract is in
// mi355_clenabled.h.  A sync_decimator by subint_len: input 0 carries time samples of num_rows num_channels floats, the optional input
// 1 the num_rows time-flag bytes of each sample (clFilterbankCleaner's output 1); an output item is one sub-integration of num_rows
// nbin num_channels floats ([row][bin][chan]), the optional output 1 its num_rows nbin hit counts (uint32).  models: 3 num_rows words,
// row-major.  The input message port "models" takes a pair whose cdr is a u64vector of 3 num_rows words and calls set_models; a
// message of another size is dropped.  The library handle counts the absolute sample index.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clFolder : virtual public gr::sync_decimator {
public:
    typedef std::shared_ptr<clFolder> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels, int nbin, int subint_len,
                     const std::vector<uint64_t> &models, int setDebug = 0);
    virtual void set_models(const std::vector<uint64_t> &models) = 0;  // 3 num_rows words, anything else throws; for the calls after it returns
    virtual std::vector<uint64_t> models() const = 0;
    virtual uint64_t sample() const = 0;          // the absolute index of the next sample
    virtual void set_sample(uint64_t T) = 0;
    virtual void skip(long long n) = 0;           // n >= 0 samples that are not folded
    virtual int nbin() const = 0;
    virtual int subint_len() const = 0;
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clPeriodSearch -- exact fast-folding search (FFA) for pulsars of unknown period behind clDedisperser's per-trial output:
// per series and base period p_lo <= p <= p_hi the first 2^log2_rows p samples as 2^log2_rows rows of p bins, combined by the FFA's fixed
// tree of binary32 additions into the profiles of the trial periods p + i / (2^log2_rows - 1), each searched with num_widths circular
// dyadic boxcars normalised to S/N.  Beyond the reference module; the contract is in mi355_clenabled.h.  A sync_block: an input item is
// one whole segment of num_series series of segment_len() = 2^log2_rows p_hi floats (series-major), an output item the num_series
// records_per_series() peak records of 8 bytes ({float snr; uint32 loc = (k << 24) | j}, [series][p - p_lo][i]); the optional output 1
// carries the profiles, p_hi floats per record, of which the floats j >= p are not written.  mean / inv_sigma: num_series floats each
// (what mi355_psearch_measure returns); empty vectors at make() are mean 0 and inv_sigma 1.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clPeriodSearch : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clPeriodSearch> sptr;
    struct peak {
        float snr;
        uint32_t loc;
    };
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int p_lo, int p_hi, int log2_rows,
                     int num_widths, const std::vector<float> &mean = std::vector<float>(), const std::vector<float> &inv_sigma = std::vector<float>(),
                     int setDebug = 0);
    virtual void set_stats(const std::vector<float> &mean, const std::vector<float> &inv_sigma) = 0;  // num_series entries each, anything else throws
    virtual std::vector<float> mean() const = 0;
    virtual std::vector<float> inv_sigma() const = 0;
    virtual long long segment_len() const = 0;         // samples per series of an input item: 2^log2_rows p_hi
    virtual long long records_per_series() const = 0;  // (p_hi - p_lo + 1) 2^log2_rows
    virtual double period(int p, int i, double tsamp_s) const = 0;  // seconds, what mi355_fold_model takes; NaN outside the ranges
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clSpectralSearch -- FFT periodicity search with exact harmonic sums behind clDedisperser's per-trial output: every
// series of n samples (a power of two, 2^8 .. 2^22) is transformed into its normalised power spectrum of n / 2 bins (zero below k_lo),
// level h <= num_folds adds the 2^h - 1 lower harmonics of every bin in a pinned order of binary32 additions, and every block of
// block_bins bins gives the record of its largest S/N over the levels.  Beyond the reference module; the contract is in
// mi355_clenabled.h.  A sync_block: an input item is one whole segment of num_series series of n floats (series-major), an output item
// the num_series records_per_series() peak records of 8 bytes ({float snr; uint32 loc = (h << 24) | k_in_block}, [series][block]); the
// optional output 1 carries the spectra, n / 2 floats per series.  inv_sigma: num_series floats (what mi355_psearch_measure returns);
// an empty vector at make() is 1.  Candidates are not exposed here: there is no message port.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clSpectralSearch : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clSpectralSearch> sptr;
    struct peak {
        float snr;
        uint32_t loc;
    };
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int n, int num_folds, int block_bins,
                     int k_lo = 1, const std::vector<float> &inv_sigma = std::vector<float>(), int setDebug = 0);
    virtual void set_stats(const std::vector<float> &inv_sigma) = 0;  // num_series entries, anything else throws
    virtual std::vector<float> inv_sigma() const = 0;
    virtual long long segment_len() const = 0;         // samples per series of an input item: n
    virtual long long num_bins() const = 0;            // n / 2
    virtual long long records_per_series() const = 0;  // n / 2 / block_bins
    virtual double freq(int h, int k, double tsamp_s) const = 0;  // Hz, the fundamental of bin k of level h; NaN outside the ranges
    virtual void set_generic(bool on) = 0;  // the generic route for every later call
    virtual std::string route() const = 0;
};

// gr::clenabled::clAccelResampler -- exact acceleration trials behind clDedisperser's per-trial output: every series of n 32-bit words
// (256 .. 2^22, any integer) is stretched quadratically once per trial with the integer index src_a(i) = i + floor((c[a] i (n - i) +
// 2^63) / 2^64); the words are moved, never computed on.  Beyond the reference module; the contract is in mi355_clenabled.h.  A
// sync_block: an input item is one whole segment of num_series series of n floats (series-major), an output item its rows()
// = num_series x num_trials() series of n floats, [series][trial] -- what clSpectralSearch takes as rows() series.  trials: one signed
// 64-bit coefficient per trial in 2^-64 sample per sample^2 (mi355_accel_coeff, mi355_accel_trials), at least one, |c| n <= 2^63.
// (No per-block header of this name is installed by this build yet.)
class CLENABLED_API clAccelResampler : virtual public gr::sync_block {
public:
    typedef std::shared_ptr<clAccelResampler> sptr;
    static sptr make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int n,
                     const std::vector<long long> &trials, int setDebug = 0);
    virtual void set_trials(const std::vector<long long> &trials) = 0;  // num_trials() entries, anything else throws
    virtual std::vector<long long> trials() const = 0;
    virtual long long segment_len() const = 0;  // samples per series of an input item: n
    virtual long long num_trials() const = 0;
    virtual long long rows() const = 0;         // series of an output item: num_series x num_trials()
    virtual void set_generic(bool on) = 0;      // the generic route for every later call
    virtual std::string route() const = 0;
};

}  // namespace clenabled
}  // namespace gr
