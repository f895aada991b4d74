// test-clenabled-mi355: standalone timing harness for the hot-path blocks, the counterpart of the
// reference's test-clenabled / test-clenabled-fft / test-clfilter / test-clxengine tools
// (lib/test_clenabled.cc:1562-1691, lib/test-clenabled-fft.cc:54-92, lib/test-clfilter.cc:88-366,
// lib/test-clxengine.cc:175-548).  Method as in the reference's study: each block in isolation,
// 1 untimed warm-up + N timed calls with std::chrono::steady_clock, host buffers in and out
// (so every figure includes H2D and D2H).  Every block's output is also checked against the
// closed-form answer the reference's own tools use, and the program exits non-zero on a mismatch.
#include <clenabled/clenabled.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace gr::clenabled;

static int g_dev = 0, g_iter = 100, g_fail = 0;

template <class F> static double time_calls(F &&fn)
{
    fn();  // warm-up
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < g_iter; i++) fn();
    std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
    return dt.count() / g_iter;
}

static void report(const char *name, size_t nsamples, double sec, bool ok)
{
    printf("%-44s %10.1f us/call  %10.2f MSPS  %s\n", name, sec * 1e6, nsamples / sec / 1e6, ok ? "ok" : "MISMATCH");
    if (!ok) g_fail++;
}

static bool close_to(gr_complex a, gr_complex b, float tol) { return std::abs(a - b) <= tol; }

static void test_math(size_t n)
{
    std::vector<gr_complex> a(n, gr_complex(1.0f, 0.5f)), b(n, gr_complex(1.0f, 0.5f)), c(n);  // lib/test_clenabled.cc:1596-1600
    gr_vector_const_void_star in = {a.data(), b.data()};
    gr_vector_void_star out = {c.data()};
    gr_vector_int ni;
    auto mul = clMathOp::make(DTYPE_COMPLEX, OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, MATHOP_MULTIPLY);
    double t = time_calls([&] { mul->testOpenCL((int)n, ni, in, out); });
    report("clMathOp multiply (complex)", n, t, c[0] == gr_complex(0.75f, 1.0f) && c[n - 1] == gr_complex(0.75f, 1.0f));
    auto mc = clMathConst::make(DTYPE_COMPLEX, OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 2.0f, MATHOP_MULTIPLY);
    gr_vector_const_void_star in1 = {a.data()};
    t = time_calls([&] { mc->testOpenCL((int)n, ni, in1, out); });
    report("clMathConst multiply by 2 (complex)", n, t, c[0] == gr_complex(2.0f, 1.0f));  // :1351-1356
}

static void test_fft(int fft_size, size_t n)
{
    n = n / fft_size * fft_size;
    if (n == 0) n = fft_size;
    std::vector<gr_complex> x(n), y(n);
    for (size_t i = 0; i < n; i++) {  // one-cycle tone per frame, lib/clFFT_impl.cc:369-377
        double ph = 2 * M_PI * (double)(i % fft_size) / fft_size;
        x[i] = gr_complex((float)sin(ph), (float)cos(ph));
    }
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    auto f = clFFT::make(fft_size, CLFFT_FORWARD, {}, DTYPE_COMPLEX, OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev);
    double t = time_calls([&] { f->testOpenCL((int)n, in, out); });
    bool ok = close_to(y[fft_size - 1], gr_complex(0.0f, (float)fft_size), 1e-3f * fft_size);  // X[N-1] = (0, N)
    float other = 0;
    for (int k = 0; k < fft_size - 1; k++) other = std::max(other, std::abs(y[k]));
    char name[64];
    snprintf(name, sizeof name, "clFFT forward N=%d", fft_size);
    report(name, n, t, ok && other < 1e-3f * fft_size);
}

static void test_filter(int ntaps, size_t n)
{
    std::vector<float> taps(ntaps);
    for (int i = 0; i < ntaps; i++) taps[i] = (i + 1) / 1000.0f;  // lib/test-clfilter.cc:98-100
    std::vector<gr_complex> x(n + ntaps - 1, gr_complex(0, 0)), y(n);
    x[ntaps - 1 + 10] = gr_complex(1.0f, 2.0f);  // impulse at sample 10 (history-prefixed buffer)
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    for (int use_time = 0; use_time < 2; use_time++) {
        auto f = clFilter::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 1, taps, 1, 0, use_time != 0);
        double t = time_calls([&] { f->testOpenCL((int)n, in, out); });
        bool ok = true;
        for (int k = 0; k < ntaps && 10 + k < (int)n; k++) ok = ok && close_to(y[10 + k], taps[k] * gr_complex(1.0f, 2.0f), 2e-5f);
        char name[64];
        snprintf(name, sizeof name, "clFilter %d taps, %s", ntaps, use_time ? "time domain" : "frequency domain");
        report(name, n, t, ok && close_to(y[0], gr_complex(0, 0), 2e-5f));
    }
}

static void test_pfb()
{
    const int M = 64, K = 2048, buf = 65536;
    std::vector<float> taps(K, 0.0f);
    for (int j = 0; j < M; j++) taps[j] = 1.0f;  // first tap of every arm = 1: y_i[c] = M-point IDFT of one input row
    std::vector<int> chmap(M);
    for (int c = 0; c < M; c++) chmap[c] = c;
    std::vector<gr_complex> x(buf + K - M), y(buf);
    for (size_t i = 0; i < x.size(); i++) x[i] = gr_complex(i % M == (size_t)((K - 1) % M) ? 1.0f : 0.0f, 0.0f);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    gr_vector_int ni;
    auto p = clPolyphaseChannelizer::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, taps, buf, M, M, chmap);
    double t = time_calls([&] { p->general_work(buf, ni, in, out); });
    // only arm 0 sees the ones (buf[i*M + K-1] == 1, tap 0) -> v_i = delta[0] -> every channel = 1
    bool ok = true;
    for (int c = 0; c < M; c++) ok = ok && close_to(y[5 * M + c], gr_complex(1.0f, 0.0f), 1e-5f);
    report("clPolyphaseChannelizer 64 ch, buf_items 65536", buf, t, ok);
}

static void test_xengine(int nant, int nchan, int ntime)
{
    auto xe = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, nant, CLXCORR_TRIANGULAR_ORDER, 0,
                              nchan, ntime, {});
    std::vector<char> x((size_t)xe->get_input_buffer_size() * 2);
    for (size_t i = 0; i < x.size(); i += 2) { x[i] = 127; x[i + 1] = 0; }  // every sample (127,0) -> every visibility = T
    std::vector<XComplex> v(xe->get_output_buffer_size());
    int save = g_iter;
    g_iter = std::max(1, g_iter / 10);
    double t = time_calls([&] { xe->xcorrelate(x.data(), v.data()); });
    g_iter = save;
    bool ok = true;
    for (size_t i = 0; i < v.size(); i += 997) ok = ok && std::fabs(v[i].real - ntime) < 1e-3f * ntime && v[i].imag == 0.0f;
    char name[80];
    snprintf(name, sizeof name, "clXEngine %d ant x %d ch x %d frames (IChar)", nant, nchan, ntime);
    report(name, (size_t)nant * nchan * ntime, t, ok);
}

// Streams frames through clXEngine::work_test() the way the scheduler would (ragged call sizes), with the file
// sink + JSON sidecar + MB rollover (lib/clXEngine_impl.cc:393-465,1259-1277) and with the result handler that
// stands for the "xcorr" PDU port.  Known answer: every sample (127,0) -> every visibility = T.
static size_t g_handler_calls = 0;
static bool g_handler_ok = true;
static void on_matrix(void *user, const XComplex *m, size_t n)
{
    const int T = *(int *)user;
    g_handler_calls++;
    for (size_t i = 0; i < n; i += 13) g_handler_ok = g_handler_ok && std::fabs(m[i].real - T) < 1e-3f * T && m[i].imag == 0.0f;
}

static int xengine_stream_test(const std::string &dir)
{
    const int N = 8, F = 64, T = 16, nint = 60, chunk = 7;
    std::vector<char> stream((size_t)(nint * T + 8) * F * 2);  // (+ the frames of the unfinished window of the first run)
    for (size_t i = 0; i < stream.size(); i += 2) { stream[i] = 127; stream[i + 1] = 0; }
    auto run = [&](clXEngine::sptr xe, int frames_total) {
        gr_vector_void_star out;
        int done = 0;
        while (done < frames_total) {
            gr_vector_const_void_star in(N);
            for (int a = 0; a < N; a++) in[a] = stream.data() + (size_t)done * F * 2;
            int want = std::min(chunk, frames_total - done);
            done += xe->work_test(want, in, out);  // may consume fewer than offered at a window boundary (:925-934)
        }
        xe->stop();
    };
    int T_user = T;
    {   // PDU-style delivery
        auto xe = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {});
        xe->set_result_handler(on_matrix, &T_user);
        run(xe, nint * T + 5);  // 5 frames of an unfinished window are never delivered
        bool ok = g_handler_calls == (size_t)nint && g_handler_ok && xe->integrations_delivered() == nint;
        report("clXEngine work_test -> result handler (60 windows)", (size_t)nint * T * F * N, 1.0, ok);
    }
    {   // file sink with 1 MB rollover + JSON sidecars
        auto xe = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 100, F, T,
                                  {"a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7"}, true, dir + "/xcorr", 1, false, 1234567, "3C286", 1.4e9,
                                  250e3);
        run(xe, nint * T);
        report("clXEngine work_test -> file sink, rollover 1 MB", (size_t)nint * T * F * N, 1.0, xe->integrations_delivered() == nint);
    }
    {   // pipeline integration: 3 device windows per delivered matrix -> values 3T
        T_user = 3 * T;
        g_handler_calls = 0;
        auto xe = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {},
                                  false, "", 0, false, 0, "", 0.0, 0.0, false, 3);
        xe->set_result_handler(on_matrix, &T_user);
        run(xe, 9 * T);
        report("clXEngine pipeline_integration=3 (9 windows -> 3)", (size_t)9 * T * F * N, 1.0, g_handler_calls == 3 && g_handler_ok);
    }
    {   // the same block over four ranks of this process (here: all on the one device): antenna groups in, channel slabs out, the matrices
        // identical to the one-device block's -- random samples this time, compared value by value
        std::vector<char> rnd((size_t)T * N * F * 2);
        unsigned lcg = 12345u;
        for (auto &c : rnd) { lcg = lcg * 1664525u + 1013904223u; c = (char)(lcg >> 24); }
        auto one = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {});
        auto four = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {});
        four->set_shard_devices({g_dev, g_dev, g_dev, g_dev});
        std::vector<XComplex> a((size_t)one->get_output_buffer_size()), b(a.size());
        one->xcorrelate(rnd.data(), a.data());
        four->xcorrelate(rnd.data(), b.data());
        bool ok = four->shard_devices() == 4 && memcmp(a.data(), b.data(), a.size() * sizeof(XComplex)) == 0;
        // and through the streaming entry: windows of constant samples, the handler's check
        T_user = T;
        g_handler_calls = 0;
        g_handler_ok = true;
        four->set_result_handler(on_matrix, &T_user);
        // 11 windows = two exchanges of four (pinned slots, one exchange in flight under the gather of the next) + three that stop() flushes
        run(four, 11 * T);
        ok = ok && g_handler_calls == 11 && g_handler_ok && four->integrations_delivered() == 11;
        // the same with one and with three windows per exchange, on two ranks
        for (int wpe : {1, 3}) {
            auto two = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {});
            two->set_shard_devices({g_dev, g_dev}, wpe);
            g_handler_calls = 0;
            two->set_result_handler(on_matrix, &T_user);
            run(two, 7 * T + 3);
            ok = ok && g_handler_calls == 7 && g_handler_ok && two->integrations_delivered() == 7;
        }
        report("clXEngine over 4 / 2 ranks of one process (set_shard_devices), streamed", (size_t)26 * T * F * N, 1.0, ok);
    }
    return g_fail ? 1 : 0;
}

static void test_elem(size_t n)
{
    // known answers for the remaining elementwise family (kernels: lib/clLog_impl.cc:113-147, clSNR_impl.cc:98-116,
    // clComplexToMag_impl.cc:138-148, clComplexToArg_impl.cc:136-151, clMagPhaseToComplex_impl.cc:170-191,
    // clQuadratureDemod_impl.cc:118-146)
    const int G = OCLTYPE_GPU, S = OCLDEVICESELECTOR_SPECIFIC;
    std::vector<float> fa(n, 100.0f), fb(n, 10.0f), fo(n), fo2(n);
    std::vector<gr_complex> ca(n + 1), co(n);
    for (size_t i = 0; i <= n; i++) ca[i] = gr_complex(3.0f, 4.0f);
    auto near = [](float a, float b) { return std::fabs(a - b) <= 1e-5f * std::max(1.0f, std::fabs(b)); };
    {
        gr_vector_const_void_star in = {fa.data()}; gr_vector_void_star out = {fo.data()};
        auto b = clLog::make(G, S, 0, g_dev, 10.0f, 0.0f);
        double t = time_calls([&] { b->testOpenCL((int)n, in, out); });
        report("clLog 10*log10(100)", n, t, near(fo[0], 20.0f) && near(fo[n - 1], 20.0f));
    }
    {
        gr_vector_const_void_star in = {fa.data(), fb.data()}; gr_vector_void_star out = {fo.data()};
        auto b = clSNR::make(G, S, 0, g_dev, 10.0f, 0.0f);
        double t = time_calls([&] { b->testOpenCL((int)n, in, out); });
        report("clSNR |10*log10(100/10)|", n, t, near(fo[0], 10.0f) && near(fo[n - 1], 10.0f));
    }
    {
        gr_vector_const_void_star in = {ca.data()}; gr_vector_void_star out = {fo.data()};
        auto b = clComplexToMag::make(G, S, 0, g_dev);
        double t = time_calls([&] { b->testOpenCL((int)n, in, out); });
        report("clComplexToMag |(3,4)|", n, t, near(fo[0], 5.0f) && near(fo[n - 1], 5.0f));
        auto a = clComplexToArg::make(G, S, 0, g_dev);
        t = time_calls([&] { a->testOpenCL((int)n, in, out); });
        report("clComplexToArg arg(3,4)", n, t, near(fo[0], atan2f(4.0f, 3.0f)) && near(fo[n - 1], atan2f(4.0f, 3.0f)));
        gr_vector_void_star out2 = {fo.data(), fo2.data()};
        auto mp = clComplexToMagPhase::make(G, S, 0, g_dev);
        t = time_calls([&] { mp->testOpenCL((int)n, in, out2); });
        report("clComplexToMagPhase (3,4)", n, t, near(fo[n - 1], 5.0f) && near(fo2[n - 1], atan2f(4.0f, 3.0f)));
    }
    {
        std::vector<float> mag(n, 2.0f), ph(n, (float)M_PI_2);
        gr_vector_const_void_star in = {mag.data(), ph.data()}; gr_vector_void_star out = {co.data()};
        auto b = clMagPhaseToComplex::make(G, S, 0, g_dev);
        double t = time_calls([&] { b->testOpenCL((int)n, in, out); });
        report("clMagPhaseToComplex (2, pi/2)", n, t, close_to(co[0], gr_complex(0.0f, 2.0f), 1e-5f) && close_to(co[n - 1], gr_complex(0.0f, 2.0f), 1e-5f));
    }
    {
        for (size_t i = 0; i <= n; i++) ca[i] = gr_complex((float)cos(0.1 * (double)i), (float)sin(0.1 * (double)i));
        gr_vector_const_void_star in = {ca.data()}; gr_vector_void_star out = {fo.data()};
        auto b = clQuadratureDemod::make(2.0f, G, S, 0, g_dev);  // history 2: n outputs read n+1 inputs
        double t = time_calls([&] { b->testOpenCL((int)n, in, out); });
        report("clQuadratureDemod gain 2, 0.1 rad/sample", n, t, std::fabs(fo[0] - 0.2f) < 1e-4f && std::fabs(fo[n - 1] - 0.2f) < 1e-4f && b->history() == 2);
    }
}

static void test_xcorr(int fft_size, size_t n)
{
    // impulse at 0 against impulses delayed by d: |IFFT(X0 conj Xs)| = N at lag -d, which the half swap moves to N/2 - d
    const int nframes = (int)std::max<size_t>(1, n / fft_size), d1 = 5, d2 = 100 % fft_size;
    std::vector<gr_complex> x0((size_t)nframes * fft_size), x1(x0.size()), x2(x0.size());
    std::vector<float> y1(x0.size()), y2(x0.size());
    for (int f = 0; f < nframes; f++) {
        x0[(size_t)f * fft_size] = 1.0f;
        x1[(size_t)f * fft_size + d1] = 1.0f;
        x2[(size_t)f * fft_size + d2] = 1.0f;
    }
    gr_vector_const_void_star in = {x0.data(), x1.data(), x2.data()};
    gr_vector_void_star out = {y1.data(), y2.data()};
    auto b = clxcorrelate_fft_vcf::make(fft_size, 3, OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 2);
    double t = time_calls([&] { b->work_test(nframes, in, out); });
    bool ok = true;
    const size_t last = (size_t)(nframes - 1) * fft_size;
    for (int k = 0; k < fft_size; k++) {
        const float e1 = (k == fft_size / 2 - d1) ? (float)fft_size : 0.0f, e2 = (k == (fft_size / 2 - d2 + fft_size) % fft_size) ? (float)fft_size : 0.0f;
        ok = ok && std::fabs(y1[last + k] - e1) < 1e-3f * fft_size && std::fabs(y2[k] - e2) < 1e-3f * fft_size;
    }
    char name[64];
    snprintf(name, sizeof name, "clxcorrelate_fft_vcf N=%d, 3 inputs", fft_size);
    report(name, (size_t)nframes * fft_size, t, ok);
}

// End-to-end streaming rate of BASELINE config 5 through the block interface, the measurement of the reference's
// test-clxengine (lib/test-clxengine.cc:287-332): one frame per work_test() call on every input, host buffers,
// frames gathered into the pinned slot, H2D + correlation + D2H overlapped with the gather of the next window.
#ifndef MI355_WITH_GNURADIO
template <class B> static void drain_messages(B &blk)  // the subscriber of the "xcorr" port: takes every message, drops it
{
    gr::shim_message m;
    while (blk->pop_message(m)) {}
}
#else
template <class B> static void drain_messages(B &) {}
#endif

static int xengine_e2e(int nint)
{
    const int N = 64, F = 1024, T = 1024;
    auto xe = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {});
    int T_user = T;
    g_handler_calls = 0;
    xe->set_result_handler(on_matrix, &T_user);
    std::vector<char> frame((size_t)F * 2);
    for (size_t i = 0; i < frame.size(); i += 2) { frame[i] = 127; frame[i + 1] = 0; }
    gr_vector_const_void_star in(N, frame.data());
    gr_vector_void_star out;
    for (int t = 0; t < 2 * T; t++) xe->work_test(1, in, out);  // two warm-up windows (each allocates its slot)
    drain_messages(xe);
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < nint; i++) {
        for (int t = 0; t < T; t++) xe->work_test(1, in, out);
        drain_messages(xe);
    }
    xe->stop();
    drain_messages(xe);
    std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
    const double per = dt.count() / nint;
    printf("clXEngine e2e 64 ant x 1024 ch x 1024 frames, 1 frame per work_test call: %.2f ms per integration, "
           "%.1f MSPS total input, %.2f MSPS per stream, %.2f Gbit/s in\n",
           per * 1e3, (double)N * F * T / per / 1e6, (double)F * T / per / 1e6, (double)N * F * T * 16 / per / 1e9);
    bool ok = g_handler_calls == (size_t)nint + 2 && g_handler_ok;
    // the same stream in scheduler-sized calls of 256 frames per input (what a GNU Radio work() call carries): the frame
    // gather is split over the helper pool
    {
        const int per_call = 256;
        auto xe2 = clXEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {});
        g_handler_calls = 0;
        xe2->set_result_handler(on_matrix, &T_user);
        std::vector<char> frames((size_t)F * 2 * per_call);
        for (size_t i = 0; i < frames.size(); i += 2) { frames[i] = 127; frames[i + 1] = 0; }
        gr_vector_const_void_star in2(N, frames.data());
        for (int t = 0; t < 2 * T; t += per_call) xe2->work_test(per_call, in2, out);
        drain_messages(xe2);
        auto t1 = std::chrono::steady_clock::now();
        double pos_ms[4] = {0, 0, 0, 0};  // time by position of the call inside its window (the last one also submits and collects)
        for (int i = 0; i < nint; i++) {
            for (int t = 0; t < T; t += per_call) {
                auto c0 = std::chrono::steady_clock::now();
                xe2->work_test(per_call, in2, out);
                pos_ms[(t / per_call) & 3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
            }
            drain_messages(xe2);
        }
        xe2->stop();
        drain_messages(xe2);
        printf("  ms per call by position in the window: %.2f %.2f %.2f %.2f\n", pos_ms[0] / nint, pos_ms[1] / nint, pos_ms[2] / nint, pos_ms[3] / nint);
        std::chrono::duration<double> d2 = std::chrono::steady_clock::now() - t1;
        const double per2 = d2.count() / nint;
        printf("clXEngine e2e 64 ant x 1024 ch x 1024 frames, %d frames per work_test call: %.2f ms per integration, "
               "%.1f MSPS total input, %.2f MSPS per stream, %.2f Gbit/s in\n",
               per_call, per2 * 1e3, (double)N * F * T / per2 / 1e6, (double)F * T / per2 / 1e6, (double)N * F * T * 16 / per2 / 1e9);
        ok = ok && g_handler_calls == (size_t)nint + 2 && g_handler_ok;
    }
    printf("%s\n", ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

// The blocks against a caller acting as the GNU Radio scheduler (stand-alone build: the scaffold of gr_compat.h records what a
// block asks of the scheduler): io signatures, history / output multiple, consume counts of general_work(), the X-engine's
// "xcorr" / "sync" message ports and its stream-tag synchroniser (lib/clXEngine_impl.cc:1152-1232).
static int scheduler_contract_test()
{
#ifdef MI355_WITH_GNURADIO
    printf("scheduler contract: run inside a GNU Radio flowgraph instead\n");
    return 0;
#else
    const int G = OCLTYPE_GPU, S = OCLDEVICESELECTOR_SPECIFIC;
    int fails = 0;
    auto check = [&](bool ok, const char *what) { printf("%-78s %s\n", what, ok ? "ok" : "MISMATCH"); if (!ok) fails++; };
    {
        auto m = clMathOp::make(DTYPE_COMPLEX, G, S, 0, g_dev, MATHOP_MULTIPLY);
        check(m->input_signature()->min_streams() == 2 && m->input_signature()->max_streams() == 2 && m->input_signature()->sizeof_stream_item(0) == 8 &&
                  m->output_signature()->max_streams() == 1, "clMathOp io signature: 2 x complex in, 1 x complex out");
        auto f = clFFT::make(1024, CLFFT_FORWARD, std::vector<float>(), DTYPE_FLOAT, G, S, 0, g_dev, 0, 3, false);
        check(f->input_signature()->max_streams() == 3 && f->input_signature()->sizeof_stream_item(0) == 4096 && f->output_signature()->sizeof_stream_item(0) == 8192,
              "clFFT io signature: num_streams vectors, float in / complex out");
        auto d = clFilter::make(G, S, 0, g_dev, 4, std::vector<float>(65, 0.01f));
        check(d->history() == 65 && d->decimation() == 4, "clFilter history = taps, sync_decimator decimation");
    }
    {   // polyphase channelizer: k output multiples per general_work() call
        const int M = 8, tpa = 4, buf = M * 32, k = 3;
        std::vector<float> taps((size_t)M * tpa);
        for (size_t i = 0; i < taps.size(); i++) taps[i] = 0.01f * (float)(i % 7) - 0.02f;
        std::vector<int> map(M);
        for (int i = 0; i < M; i++) map[i] = i;
        auto p = clPolyphaseChannelizer::make(G, S, 0, g_dev, taps, buf, M, M, map);
        check(p->history() == taps.size() && p->output_multiple() == buf, "clPolyphaseChannelizer history = taps, output multiple = items per buffer");
        std::vector<gr_complex> x((size_t)k * buf + taps.size() - M), y1((size_t)k * buf), yk(y1.size());
        for (size_t i = 0; i < x.size(); i++) x[i] = gr_complex((float)std::sin(0.37 * (double)i), (float)std::cos(0.11 * (double)i));
        gr_vector_int ninput(1, (int)x.size());
        for (int b = 0; b < k; b++) {
            gr_vector_const_void_star in = {x.data() + (size_t)b * buf}; gr_vector_void_star out = {y1.data() + (size_t)b * buf};
            p->general_work(buf, ninput, in, out);
        }
        const long single = p->nitems_consumed(0);
        p->reset_consumed();
        gr_vector_const_void_star in = {x.data()}; gr_vector_void_star out = {yk.data()};
        gr_vector_int req(1, 0);
        p->forecast(k * buf, req);
        const int produced = p->general_work(k * buf, ninput, in, out);
        check(single == (long)k * buf && p->nitems_consumed(0) == (long)k * buf && produced == k * buf && req[0] == (int)x.size(),
              "clPolyphaseChannelizer general_work(k multiples): consume_each(k * buf_items), forecast");
        check(memcmp(y1.data(), yk.data(), y1.size() * sizeof(gr_complex)) == 0, "clPolyphaseChannelizer k buffers in one call == k single calls (bit exact)");
    }
    {   // X-engine: message ports and the tag synchroniser
        const int N = 4, F = 64, T = 16;
        auto xe = clXEngine::make(G, S, 0, g_dev, false, DTYPE_BYTE, 1, N, CLXCORR_TRIANGULAR_ORDER, 0, F, T, {}, false, "", 0, true /* synchroniser */);
        check(xe->message_ports_out().size() == 2 && xe->message_ports_out()[0] == "xcorr" && xe->message_ports_out()[1] == "sync" && xe->output_multiple() == 16,
              "clXEngine registers \"xcorr\" and \"sync\"; synchroniser sets output multiple 16");
        check(xe->input_signature()->min_streams() == 2 && xe->input_signature()->max_streams() == N && xe->input_signature()->sizeof_stream_item(0) == F * 2 &&
                  xe->output_signature()->max_streams() == 0, "clXEngine io signature: antennas x channel rows in, no stream out");
        std::vector<char> frames((size_t)F * 2 * 64);
        for (size_t i = 0; i < frames.size(); i += 2) { frames[i] = 127; frames[i + 1] = 0; }
        gr_vector_const_void_star in(N, frames.data());
        gr_vector_void_star out;
        gr_vector_int ninput(N, 64);
        xe->set_first_tags({1000, 1016, 1000, 1048});  // inputs 0 and 2 are 48 behind the latest, input 1 is 32 behind
        int r = xe->general_work(32, ninput, in, out);
        check(r == 0 && !xe->synchronized() && xe->nitems_consumed(0) == 32 && xe->nitems_consumed(1) == 32 && xe->nitems_consumed(2) == 32 &&
                  xe->nitems_consumed(3) == 0, "unaligned tags: nothing produced, lagging inputs advance by min(highest - own, noutput_items)");
        xe->reset_consumed();
        xe->set_first_tags({1032, 1048, 1032, 1048});
        r = xe->general_work(32, ninput, in, out);
        check(r == 0 && xe->nitems_consumed(0) == 16 && xe->nitems_consumed(1) == 0 && xe->nitems_consumed(3) == 0, "second round: the remaining 16 items");
        xe->reset_consumed();
        xe->set_first_tags({1048, 1048, 1048, 1048});
        r = xe->general_work(32, ninput, in, out);  // aligned: synchronised, then T = 16 frames of the window are taken
        gr::shim_message msg;
        const bool got_sync = xe->pop_message(msg) && msg.port == "sync" && msg.key == "synctimestamp" && msg.u64 == 1048;
        check(r == T && xe->synchronized() && xe->sync_tag() == 1048 && got_sync && xe->nitems_consumed(0) == T && xe->nitems_consumed(3) == T,
              "aligned tags: \"sync\" message (synctimestamp, 1048), work proceeds, consume_each(items)");
        for (int i = 0; i < 3; i++) xe->general_work(T, ninput, in, out);
        xe->stop();
        int nmsg = 0;
        bool ok = true;
        const size_t len = (size_t)F * (N * (N + 1) / 2);
        while (xe->pop_message(msg)) {
            nmsg++;
            ok = ok && msg.port == "xcorr" && msg.key == "triang_matrix" && msg.c32.size() == len && std::fabs(msg.c32[0].real() - (float)T) < 1e-3f &&
                 std::fabs(msg.c32[len - 1].real() - (float)T) < 1e-3f && msg.c32[5].imag() == 0.0f;
        }
        check(nmsg == 4 && ok, "\"xcorr\" messages: (triang_matrix, c32vector of nchan * nbaselines) per integration");
    }
    printf("%s\n", fails ? "MISMATCH" : "ok");
    return fails ? 1 : 0;
#endif
}

// --xcorrelate-only (the reference's lib/test-clxcorrelate.cc:349 options: --num_inputs=, --maxsearch=, --input_complex, size):
// time per work() call of clXCorrelate, and a known answer -- input s is input 0 delayed by 3 s + 1 samples, so its lag is -(3 s + 1)
static int xcorrelate_test(size_t n, int num_inputs, int maxsearch, bool cplx)
{
#ifdef MI355_WITH_GNURADIO
    (void)n; (void)num_inputs; (void)maxsearch; (void)cplx;
    printf("--xcorrelate-only reads the published PDUs of the stand-alone build\n");
    return 2;
#else
    const int dt = cplx ? DTYPE_COMPLEX : DTYPE_FLOAT, ds = cplx ? 8 : 4;
    auto b = clXCorrelate::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, false, num_inputs, (int)n, dt, ds, maxsearch, 1, false);
    const int delay_max = 3 * (num_inputs - 1) + 1;
    std::vector<float> base((n + delay_max) * (cplx ? 2 : 1));
    uint32_t seed = 12345u;
    for (auto &v : base) { seed = seed * 1664525u + 1013904223u; v = (float)((seed >> 8) & 0xffff) / 65536.0f - 0.5f; }
    gr_vector_const_void_star in(num_inputs);
    gr_vector_void_star out;
    const size_t w = cplx ? 2 : 1;
    in[0] = base.data() + delay_max * w;
    for (int s = 1; s < num_inputs; s++) in[s] = base.data() + (delay_max - (3 * s + 1)) * w;  // y[j] = x[j - d]
    const double sec = time_calls([&] { b->work((int)n, in, out); });
    gr::shim_message msg, last;
    int count = 0;
    while (b->pop_message(msg)) { last = msg; count++; }
    bool ok = count == g_iter + 1 && last.port == "corr" && (int)last.f32.size() == num_inputs - 1 && (int)last.s32.size() == num_inputs - 1;
    for (int s = 1; ok && s < num_inputs; s++) ok = last.s32[s - 1] == -(3 * s + 1) && std::fabs(last.f32[s - 1] - 1.0f) < 1e-4f;
    char name[128];
    snprintf(name, sizeof name, "clXCorrelate N=%zu, %d %s inputs, max shift %d", n, num_inputs, cplx ? "complex" : "float", b->max_shift());
    printf("%-60s %10.1f us/call  %s\n", name, sec * 1e6, ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
#endif
}

// --loops-only: time per work() call and a known answer for the NCO and the carrier loop.  clSignalSource at samp_rate / 8 steps
// pi/4 per item and every call of a multiple of 8 items starts at a multiple of 2 pi: items 1 and 2 are A (cos, sin)(pi/4) and
// (0, A).  clCostasLoop gets one QPSK point turning at 0.01 rad/item: locked, the output rests on a constellation point
// (+-1, +-1)/sqrt 2 and the loop frequency is the offset.
static int loops_test(size_t n)
{
    n = (n + 7) / 8 * 8;
    const float A = 2.5f;
    std::vector<gr_complex> y(n);
    gr_vector_const_void_star none;
    gr_vector_void_star out = {y.data()};
    auto src = clSignalSource::make(DTYPE_COMPLEX, OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 8000.0, 1, 1000.0, A);
    double t = time_calls([&] { src->work((int)n, none, out); });
    const float h = A * (float)M_SQRT1_2;
    report("clSignalSource (complex, samp_rate / 8)", n, t,
           close_to(y[0], gr_complex(A, 0), 1e-4f) && close_to(y[1], gr_complex(h, h), 1e-4f) && close_to(y[2], gr_complex(0, A), 1e-4f) &&
               close_to(y[n - 1], gr_complex(h, -h), 1e-4f));
    const double offset = 0.01;
    std::vector<gr_complex> x(n);
    for (size_t i = 0; i < n; i++) {
        const double ph = M_PI / 4 + 0.3 + offset * (double)i;
        x[i] = gr_complex((float)cos(ph), (float)sin(ph));
    }
    std::vector<float> f(n);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out2 = {y.data(), f.data()};
    auto loop = clCostasLoop::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 0.0628f, 4);
    t = time_calls([&] { loop->work((int)n, in, out2); });
    const gr_complex last = y[n - 1];
    const bool on_point = n >= 2048 && std::fabs(std::fabs(last.real()) - (float)M_SQRT1_2) < 0.02f &&
                          std::fabs(std::fabs(last.imag()) - (float)M_SQRT1_2) < 0.02f;
    report("clCostasLoop (order 4, one stream)", n, t,
           on_point && std::fabs(f[n - 1] - offset) < 0.1 * offset && std::fabs(loop->get_frequency() - f[n - 1]) < 1e-6f);
    return g_fail ? 1 : 0;
}

// --resampler-only: two impulses through (L, M) = (3, 2) must reproduce the arms, y[m] = hp[2 m] + 100 hp[2 m - 15] for taps
// h[k] = k + 1 (the second impulse, at x[5], lands on the odd taps), with the stream offered to general_work() in two uneven
// pieces chained by what the block consumed; then the time per general_work() call.
static int resampler_test(size_t n)
{
#ifdef MI355_WITH_GNURADIO
    (void)n;
    printf("--resampler-only acts as the scheduler of the stand-alone build (what general_work() consumed)\n");
    return 2;
#else
    const int L = 3, M = 2, K = 11;
    std::vector<float> taps(K);
    for (int k = 0; k < K; k++) taps[k] = (float)(k + 1);
    auto rs = clRationalResampler::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, L, M, taps);
    const int hist = (int)rs->history() - 1, nx = 64;
    std::vector<gr_complex> x(hist + nx, gr_complex(0, 0)), y(nx * L / M + 8, gr_complex(-1, -1));
    x[hist + 0] = gr_complex(1, 0);
    x[hist + 5] = gr_complex(100, 0);
    auto hp = [&](long q) { return q >= 0 && q < K ? taps[q] : 0.0f; };
    long used = 0, made = 0;
    bool ok = rs->history() == 4 && rs->interpolation() == L && rs->decimation() == M && rs->taps().size() == (size_t)K;
    const auto t0 = std::chrono::steady_clock::now();
    for (int offered : {hist + 7, hist + nx}) {  // items in the buffer from the read pointer, history included
        gr_vector_int ni = {offered - (int)used};
        gr_vector_const_void_star in = {x.data() + used};
        gr_vector_void_star out = {y.data() + made};
        rs->reset_consumed();
        const int got = rs->general_work((int)(y.size() - made), ni, in, out);
        used += rs->nitems_consumed(0);
        made += got;
    }
    ok = ok && made == (long)nx * L / M && used == nx;
    for (long m = 0; m < made; m++) ok = ok && close_to(y[m], gr_complex(hp(M * m) + 100.0f * hp(M * m - 5 * L), 0), 1e-4f);
    const std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
    report("clRationalResampler (3/2, impulse -> arms)", (size_t)made, dt.count() / 2, ok);
    n = (n + L - 1) / L * L;  // a multiple of L outputs: every call starts at the same phase
    std::vector<float> lp(97, 1.0f / 97);
    auto rt = clRationalResampler::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, L, M, lp);
    gr_vector_int need(1, 0);
    rt->forecast((int)n, need);
    std::vector<gr_complex> xi(need[0], gr_complex(1.0f, 0.5f)), yo(n);
    gr_vector_const_void_star in = {xi.data()};
    gr_vector_void_star out = {yo.data()};
    int got = 0;
    const double t = time_calls([&] { got = rt->general_work((int)n, need, in, out); });
    // a constant input: every output is the input times the sum of its arm (33, 32, 32 taps of 1/97)
    report("clRationalResampler (3/2, 97 taps)", n, t,
           got == (int)n && close_to(yo[0], gr_complex(33.0f / 97, 16.5f / 97), 1e-5f) && close_to(yo[n - 1], gr_complex(1.0f, 0.5f) * (yo[n - 1].real()), 1e-5f) &&
               std::fabs(yo[n - 1].real() * 97 - std::round(yo[n - 1].real() * 97)) < 1e-3f);
    return g_fail ? 1 : 0;
#endif
}

// --synth-only: 12 channels (mixed radix) and 64 channels (power of two), a partial map, through general_work() in two uneven
// pieces chained by what the block consumed, against a host loop over the contract's two formulas in double; then the time per
// general_work() call at 64 channels.
#ifndef MI355_WITH_GNURADIO
static bool synth_case(int M, int K, const std::vector<int> &map, int nframes)
{
    const int nmap = map.empty() ? M : (int)map.size(), T = (K + M - 1) / M;
    std::vector<float> taps(K);
    for (int k = 0; k < K; k++) taps[k] = (float)(std::sin(0.37 * k + 0.2) / M);
    auto sy = clPolyphaseSynthesizer::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, taps, M, map);
    bool ok = sy->taps_per_arm() == T && sy->nmap() == nmap && sy->num_channels() == M && (int)sy->history() == (T - 1) * nmap + 1 &&
              sy->taps().size() == (size_t)K && !sy->route().empty();
    const int nin_frames = T - 1 + nframes;
    std::vector<gr_complex> x((size_t)nin_frames * nmap), y((size_t)nframes * M, gr_complex(-1, -1));
    for (size_t i = 0; i < x.size(); i++) x[i] = gr_complex((float)std::cos(0.11 * i), (float)std::sin(0.23 * i + 1.0));
    long used = 0, made = 0;
    for (int frames_offered : {3, nframes}) {  // frames in the buffer behind the history, from the start of the stream
        gr_vector_int ni = {(T - 1 + frames_offered) * nmap - (int)used};
        gr_vector_const_void_star in = {x.data() + used};
        gr_vector_void_star out = {y.data() + made};
        sy->reset_consumed();
        const int got = sy->general_work((int)(y.size() - made) + M / 2, ni, in, out);  // room that is no multiple of M: whole frames only
        used += sy->nitems_consumed(0);
        made += got;
    }
    ok = ok && made == (long)nframes * M && used == (long)nframes * nmap;
    // host loop: V per input frame, then the FIR over frames
    std::vector<std::complex<double>> V((size_t)nin_frames * M);
    for (int f = 0; f < nin_frames; f++)
        for (int r = 0; r < M; r++) {
            std::complex<double> s(0, 0);
            for (int q = 0; q < nmap; q++) {
                const int c = map.empty() ? q : map[q];
                const double a = 2.0 * M_PI * (double)((long)r * c % M) / M;
                s += std::complex<double>(x[(size_t)f * nmap + q]) * std::complex<double>(std::cos(a), std::sin(a));
            }
            V[(size_t)f * M + r] = s;
        }
    double worst = 0, scale = 0;
    for (int l = 0; l < nframes && l * (long)M < made; l++)
        for (int r = 0; r < M; r++) {
            std::complex<double> s(0, 0);
            for (int p = 0; p < T; p++) {
                const int k = r + M * p;
                if (k < K) s += (double)taps[k] * V[(size_t)(l + T - 1 - p) * M + r];
            }
            worst = std::max(worst, std::abs(s - std::complex<double>(y[(size_t)l * M + r])));
            scale = std::max(scale, std::abs(s));
        }
    return ok && scale > 0 && worst <= 1e-5 * scale;
}
#endif

static int synth_test(size_t n)
{
#ifdef MI355_WITH_GNURADIO
    (void)n;
    printf("--synth-only acts as the scheduler of the stand-alone build (what general_work() consumed)\n");
    return 2;
#else
    auto t0 = std::chrono::steady_clock::now();
    bool ok = synth_case(12, 41, {7, 0, 3, 11, 4}, 150);
    std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
    report("clPolyphaseSynthesizer (12 channels, 5 fed, 4 per arm)", 150 * 12, dt.count(), ok);
    t0 = std::chrono::steady_clock::now();
    ok = synth_case(64, 8 * 64 - 33, {}, 200);
    dt = std::chrono::steady_clock::now() - t0;
    report("clPolyphaseSynthesizer (64 channels, 8 per arm)", 200 * 64, dt.count(), ok);
    const int M = 64, T = 8;
    n = (std::max<size_t>(n, M) + M - 1) / M * M;
    std::vector<float> lp((size_t)T * M, 1.0f / M);
    auto sy = clPolyphaseSynthesizer::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, lp, M);
    gr_vector_int need(1, 0);
    sy->forecast((int)n, need);
    // channel 0 alone carries a constant: every output is that constant times the sum of its arm, T / M
    std::vector<gr_complex> xi(need[0], gr_complex(0, 0)), yo(n);
    for (size_t i = 0; i < xi.size(); i += M) xi[i] = gr_complex(1.0f, 0.5f);
    gr_vector_const_void_star in = {xi.data()};
    gr_vector_void_star out = {yo.data()};
    int got = 0;
    const double t = time_calls([&] { got = sy->general_work((int)n, need, in, out); });
    report("clPolyphaseSynthesizer (64 channels, 8 per arm, timing)", n, t,
           got == (int)n && need[0] == (int)((T - 1 + n / M) * M) && close_to(yo[0], gr_complex(T * 1.0f / M, T * 0.5f / M), 1e-5f) &&
               close_to(yo[n - 1], gr_complex(T * 1.0f / M, T * 0.5f / M), 1e-5f));
    return g_fail ? 1 : 0;
#endif
}

// --pspec-only: 64 points (fused) with overlapping Hann frames and 100 points (generic) with skipped items, through general_work() in
// two uneven pieces chained by what the block consumed, against a direct DFT in double; then the time per general_work() call at
// 1024 points, 16 frames per spectrum.
#ifndef MI355_WITH_GNURADIO
static bool pspec_case(int N, int K, int H, bool hann, bool shift, int nspectra)
{
    std::vector<float> w;
    if (hann)
        for (int i = 0; i < N; i++) w.push_back((float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / N)));
    auto ps = clPowerSpectrum::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, N, K, w, H, shift, false, 0.5f);
    bool ok = ps->fft_size() == N && ps->navg() == K && ps->hop() == H && (int)ps->history() == std::max(N - H, 0) + 1 && !ps->route().empty();
    // what the library reads, or with hop > fft_size what the block consumes: it waits for the skipped items of a spectrum
    const long nin = std::max(((long)nspectra * K - 1) * H + N, (long)nspectra * K * H);
    std::vector<gr_complex> x((size_t)nin);
    std::vector<float> y((size_t)nspectra * N, -1.0f);
    for (size_t i = 0; i < x.size(); i++) x[i] = gr_complex((float)std::cos(0.11 * i) + 0.25f, (float)std::sin(0.23 * i + 1.0));
    long used = 0, made = 0;
    for (int offered : {2, nspectra}) {  // spectra the buffer holds, from the start of the stream
        gr_vector_int ni = {(int)(((long)offered * K - 1) * H + N + H / 2 - used)};  // (half a hop more than whole spectra need)
        if (ni[0] > (int)(nin - used)) ni[0] = (int)(nin - used);
        gr_vector_const_void_star in = {x.data() + used};
        gr_vector_void_star out = {y.data() + made * N};
        ps->reset_consumed();
        ps->set_offered(ni);  // consuming more than was offered throws
        const int got = ps->general_work(nspectra - (int)made, ni, in, out);
        used += ps->nitems_consumed(0);
        made += got;
    }
    ok = ok && made == nspectra && used == (long)nspectra * K * H;
    double worst = 0, scale = 0;
    for (int s = 0; s < nspectra && s < made; s++)
        for (int b = 0; b < N; b++) {
            double p = 0;
            for (int k = 0; k < K; k++) {
                std::complex<double> X(0, 0);
                const gr_complex *f = x.data() + ((size_t)s * K + k) * H;
                for (int n = 0; n < N; n++) {
                    const double a = -2.0 * M_PI * (double)((long)b * n % N) / N;
                    X += std::complex<double>(f[n]) * (hann ? (double)w[n] : 1.0) * std::complex<double>(std::cos(a), std::sin(a));
                }
                p += std::norm(X);
            }
            p *= 0.5 / K;
            const int o = shift ? (b + N / 2) % N : b;  // out[(b + floor(N / 2)) mod N] = P[b]
            worst = std::max(worst, std::abs(p - (double)y[(size_t)s * N + o]));
            scale = std::max(scale, p);
        }
    return ok && scale > 0 && worst <= 1e-5 * scale;
}
#endif

static int pspec_test(size_t n)
{
#ifdef MI355_WITH_GNURADIO
    (void)n;
    printf("--pspec-only acts as the scheduler of the stand-alone build (what general_work() consumed)\n");
    return 2;
#else
    auto t0 = std::chrono::steady_clock::now();
    bool ok = pspec_case(64, 5, 48, true, true, 6);
    std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
    report("clPowerSpectrum (64 points, 5 Hann frames, hop 48, shift)", 6 * 5 * 48, dt.count(), ok);
    t0 = std::chrono::steady_clock::now();
    ok = pspec_case(100, 3, 130, false, false, 5);
    dt = std::chrono::steady_clock::now() - t0;
    report("clPowerSpectrum (100 points, 3 frames, hop 130)", 5 * 3 * 130, dt.count(), ok);
    const int N = 1024, K = 16;
    const int S = (int)std::max<size_t>(n / ((size_t)N * K), 1);
    auto ps = clPowerSpectrum::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, N, K);
    gr_vector_int need(1, 0);
    ps->forecast(S, need);
    // a constant: all of its power in bin 0, N^2 |c|^2
    std::vector<gr_complex> xi(need[0], gr_complex(1.0f, 0.5f));
    std::vector<float> yo((size_t)S * N);
    gr_vector_const_void_star in = {xi.data()};
    gr_vector_void_star out = {yo.data()};
    int got = 0;
    const double t = time_calls([&] {
        ps->reset_consumed();
        ps->set_offered(need);  // (per call: the same buffer is offered again)
        got = ps->general_work(S, need, in, out);
    });
    const float p0 = 1.25f * N * N;
    report("clPowerSpectrum (1024 points, 16 frames, timing)", (size_t)S * N * K, t,
           got == S && need[0] == S * K * N && std::abs(yo[0] - p0) <= 1e-5f * p0 && std::abs(yo[(size_t)(S - 1) * N] - p0) <= 1e-5f * p0 &&
               std::abs(yo[1]) <= 1e-5f * p0);
    return g_fail ? 1 : 0;
#endif
}

// --xlate-only: two tones in one capture, one clFreqXlatingFIRFilter with two centre frequencies and a 32-tap boxcar whose nulls hold
// the other tone: each tone must land at DC of its own output with its own amplitude and zero phase (the phase reference is item 0 of
// the stream); then channel 0 is retuned to the second tone through the "freq" message port; then the time per work() call at
// decimation 16, 65 taps, four channels.
static int xlate_test(size_t n)
{
    const int K = 32, D = 8;
    const double fs = 1.0e6, f0 = fs / 8, f1 = -fs / 4;
    auto tone = [&](std::vector<gr_complex> &x, int hist) {
        for (size_t i = 0; i < x.size(); i++) {
            const double t = (double)i - hist;
            x[i] = gr_complex((float)(std::cos(2.0 * M_PI * f0 / fs * t) + 0.5 * std::cos(2.0 * M_PI * f1 / fs * t)),
                              (float)(std::sin(2.0 * M_PI * f0 / fs * t) + 0.5 * std::sin(2.0 * M_PI * f1 / fs * t)));
        }
    };
    const int no = 1000;
    auto fx = clFreqXlatingFIRFilter::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, D, std::vector<float>(K, 1.0f / K), {f0, f1}, fs);
    bool ok = fx->num_channels() == 2 && (int)fx->history() == K && (int)fx->decimation() == D && fx->route().compare(0, 5, "fused") == 0;
    std::vector<gr_complex> x((size_t)no * D + K - 1), y0(no, gr_complex(-9.f, -9.f)), y1(no, gr_complex(-9.f, -9.f));
    tone(x, K - 1);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y0.data(), y1.data()};
    auto t0 = std::chrono::steady_clock::now();
    ok = ok && fx->work(no, in, out) == no;
    std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
    for (int m : {0, 1, no / 2, no - 1})
        ok = ok && close_to(y0[m], gr_complex(1.0f, 0.0f), 1e-4f) && close_to(y1[m], gr_complex(0.5f, 0.0f), 1e-4f);
    report("clFreqXlatingFIRFilter (two tones, two channels, decimation 8)", (size_t)no * D, dt.count(), ok);
    // retune channel 0 to the second tone: the phase accumulator is kept, the magnitude is the second tone's
#ifdef MI355_WITH_GNURADIO
    fx->set_center_freq(f1, 0);
#else
    ok = fx->post_double("freq", f1) && !fx->post_double("nosuchport", 0.0);
#endif
    ok = ok && fx->center_freq(0) == f1 && fx->center_freq(1) == f1;
    t0 = std::chrono::steady_clock::now();
    ok = ok && fx->work(no, in, out) == no;
    dt = std::chrono::steady_clock::now() - t0;
    for (int m : {0, no - 1}) ok = ok && std::abs(std::abs(y0[m]) - 0.5f) <= 1e-4f && std::abs(std::abs(y1[m]) - 0.5f) <= 1e-4f;
    report("clFreqXlatingFIRFilter (channel 0 retuned through the freq port)", (size_t)no * D, dt.count(), ok);
    const int Dt = 16, Kt = 65, Ct = 4;
    const int nt = (int)std::max<size_t>(n / Dt, 1);
    std::vector<double> fc;
    for (int c = 0; c < Ct; c++) fc.push_back((c - 1.5) * fs / 8);
    std::vector<float> taps(Kt, 0.0f);
    taps[0] = 1.0f;  // y_c[m] = r_c(m) x[m D]
    auto ft = clFreqXlatingFIRFilter::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, Dt, taps, fc, fs);
    std::vector<gr_complex> xi((size_t)nt * Dt + Kt - 1, gr_complex(1.0f, 0.5f));
    std::vector<std::vector<gr_complex>> yo(Ct, std::vector<gr_complex>((size_t)nt));
    gr_vector_const_void_star tin = {xi.data()};
    gr_vector_void_star tout;
    for (auto &v : yo) tout.push_back(v.data());
    int got = 0;
    const double t = time_calls([&] { got = ft->work(nt, tin, tout); });
    bool tok = got == nt;
    for (int c = 0; c < Ct; c++) tok = tok && std::abs(std::abs(yo[c][nt - 1]) - std::abs(gr_complex(1.0f, 0.5f))) <= 1e-5f;
    report("clFreqXlatingFIRFilter (decimation 16, 65 taps, 4 channels, timing)", (size_t)nt * Dt, t, tok);
    return g_fail ? 1 : 0;
}

// --beamform-only: clBeamformer at (S, B, F, npol) = (20, 5, 8, 2) on frames and weights from a 32-bit linear congruential generator
// (state = 1664525 state + 1013904223, the top byte of each state; a weight of -128 becomes -127): 17 frames of voltage beams and 4
// windows of 4 frames of Stokes-I power.  Prints "checksum" lines that tests/test_beamform_gpu.py compares with the integer reference:
// voltage sum_i (i % 7 + 1) re_i + (i % 5 + 1) im_i, power sum_i (i % 7 + 1) P_i over the outputs in memory order; then one timing row.
static int beamform_test(size_t n)
{
    const int S = 20, B = 5, F = 8, npol = 2, T = 17, Ti = 4, W = 4;
    uint32_t state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return (int8_t)(state >> 24); };
    std::vector<int8_t> x((size_t)T * S * F * npol * 2), w((size_t)F * npol * B * S * 2);
    for (auto &v : x) v = next();
    for (auto &v : w) { v = next(); if (v == -128) v = -127; }
    bool ok = true;
    {
        auto bf = clBeamformer::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 0, npol, S, F, B, 1, false, w);
        ok = bf->num_beams() == B && bf->frame_bytes() == 2ll * S * F * npol && bf->decimation() == 1 && bf->route().compare(0, 4, "mfma") == 0 &&
             bf->weights() == w;
        std::vector<gr_complex> y((size_t)T * B * F * npol, gr_complex(-9.f, -9.f));
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && bf->work(T, in, out) == T;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        long long sum = 0;
        for (size_t i = 0; i < y.size(); i++) sum += (long long)(i % 7 + 1) * (long long)y[i].real() + (long long)(i % 5 + 1) * (long long)y[i].imag();
        printf("clBeamformer voltage checksum %lld\n", sum);
        report("clBeamformer (voltage, 20 inputs, 5 beams, 8 channels, 2 pol)", (size_t)T, dt.count(), ok);
    }
    {
        auto bf = clBeamformer::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 1, npol, S, F, B, Ti, true);
        bf->set_weights(w);
        bool pok = (int)bf->decimation() == Ti && bf->out_bytes_per_unit() == 4ll * B * F;
        std::vector<float> p((size_t)W * B * F, -9.f);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {p.data()};
        auto t0 = std::chrono::steady_clock::now();
        pok = pok && bf->work(W, in, out) == W;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        double sum = 0.0;
        for (size_t i = 0; i < p.size(); i++) sum += (double)(i % 7 + 1) * (double)p[i];
        printf("clBeamformer power checksum %.0f\n", sum);
        report("clBeamformer (Stokes I power, 4 windows of 4 frames)", (size_t)W * Ti, dt.count(), pok);
    }
    {
        const int St = 64, Bt = 64, Ft = 64, nt = (int)std::max<size_t>(n / 1024, 16);
        std::vector<int8_t> xt((size_t)nt * St * Ft * 2 * 2, 3), wt((size_t)Ft * 2 * Bt * St * 2, 0);
        for (size_t i = 0; i < wt.size(); i += 2) wt[i] = 1;  // every beam the plain sum of the stations
        auto bf = clBeamformer::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 0, 2, St, Ft, Bt, 1, false, wt);
        std::vector<gr_complex> y((size_t)nt * Bt * Ft * 2);
        gr_vector_const_void_star in = {xt.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = bf->work(nt, in, out); });
        report("clBeamformer (voltage, 64 x 64 x 64 x 2, timing)", (size_t)nt, t, got == nt && y.back() == gr_complex(3.f * St, 3.f * St));
    }
    return g_fail ? 1 : 0;
}

// --fengine-only: clFEngine at (S, npol, F, P) = (3, 2, 64, 2) with shift, 70 frames, on streams from the 32-bit linear congruential
// generator of --beamform-only (the top byte of each state as int8: re then im of every item, input after input), taps
// h[i] = (1 + i % 5) / 4 and all gains 1 / 512.  Prints a "checksum" line that tests/test_fengine_gpu.py compares with the float64
// reference: sum_i (i % 7 + 1) out_i over the output bytes in memory order; then one timing row.
static int fengine_test(size_t n)
{
    const int S = 3, npol = 2, F = 64, P = 2, T = 70, R = S * npol;
    const size_t items = (size_t)(T + P - 1) * F;
    uint32_t state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return (float)(int8_t)(state >> 24); };
    std::vector<std::vector<gr_complex>> x(R, std::vector<gr_complex>(items));
    for (auto &v : x)
        for (auto &c : v) { const float re = next(); const float im = next(); c = gr_complex(re, im); }
    std::vector<float> h((size_t)P * F), g((size_t)R * F, 1.0f / 512.0f);
    for (size_t i = 0; i < h.size(); i++) h[i] = (float)(1 + i % 5) * 0.25f;
    {
        auto fe = clFEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, npol, S, F, h, P, true, g);
        bool ok = fe->frame_bytes() == 2ll * S * F * npol && (int)fe->decimation() == F && (int)fe->history() == (P - 1) * F + 1 &&
                  fe->route().compare(0, 5, "fused") == 0 && fe->gains() == g;
        std::vector<int8_t> y((size_t)T * fe->frame_bytes(), -128);
        gr_vector_const_void_star in;
        for (auto &v : x) in.push_back(v.data());
        gr_vector_void_star out = {y.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && fe->work(T, in, out) == T;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        long long sum = 0;
        for (size_t i = 0; i < y.size(); i++) {
            ok = ok && y[i] != -128;
            sum += (long long)(i % 7 + 1) * (long long)y[i];
        }
        printf("clFEngine checksum %lld\n", sum);
        report("clFEngine (3 stations, 2 pol, 64 channels, 2 taps per channel)", (size_t)T, dt.count(), ok);
    }
    {
        const int St = 16, Ft = 1024, Pt = 4, nt = (int)std::max<size_t>(n / 1024, 16), Rt = St * 2;
        std::vector<gr_complex> xt((size_t)(nt + Pt - 1) * Ft, gr_complex(1.f, -1.f));
        std::vector<float> ht((size_t)Pt * Ft, 0.25f), gt((size_t)Rt * Ft, 2.0f / Ft);
        auto fe = clFEngine::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, 2, St, Ft, ht, Pt, false, gt);
        std::vector<int8_t> y((size_t)nt * fe->frame_bytes(), -128);
        gr_vector_const_void_star in(Rt, xt.data());
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = fe->work(nt, in, out); });
        // a constant 1 - j through four arms of 1/4 and a gain of 2 / F: channel 0 holds (2, -2), every other channel 0
        report("clFEngine (16 x 2 x 1024, 4 taps per channel, timing)", (size_t)nt, t, got == nt && y[0] == 2 && y[1] == -2 && y[4] == 0 && y.back() == 0);
    }
    return g_fail ? 1 : 0;
}

// --dedisp-only: clDedisperser at (R, F, D) = (2, 20, 5) with delay[d][f] = d (F - 1 - f) / 4 (max_delay 19) and channel 3 of trial 2
// killed, 70 outputs, on samples from the 32-bit linear congruential generator of --beamform-only (the top byte of each state as int8,
// as float: every sum is an exact integer).  Prints a "checksum" line that tests/test_dedisp_gpu.py compares with the numpy
// reference: sum_i (i % 7 + 1) y_i over the output floats in memory order; then one timing row.
static int dedisp_test(size_t n)
{
    const int R = 2, F = 20, D = 5, T = 70, H = (D - 1) * (F - 1) / 4;
    uint32_t state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return (float)(int8_t)(state >> 24); };
    std::vector<float> x((size_t)(T + H) * R * F);
    for (auto &v : x) v = next();
    std::vector<int32_t> tab((size_t)D * F);
    for (int d = 0; d < D; d++)
        for (int f = 0; f < F; f++) tab[(size_t)d * F + f] = d * (F - 1 - f) / 4;
    tab[2 * F + 3] = -1;
    {
        auto dd = clDedisperser::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, R, F, D, H, tab);
        bool ok = (int)dd->history() == H + 1 && dd->max_delay() == H && dd->route().compare(0, 5, "tiled") == 0 && dd->delays() == tab;
        std::vector<float> y((size_t)T * R * D, -1e30f);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && dd->work(T, in, out) == T;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        long long sum = 0;
        for (size_t i = 0; i < y.size(); i++) {
            ok = ok && y[i] != -1e30f;
            sum += (long long)(i % 7 + 1) * (long long)y[i];
        }
        printf("clDedisperser checksum %lld\n", sum);
        report("clDedisperser (2 rows, 20 channels, 5 trials)", (size_t)T, dt.count(), ok);
    }
    {
        const int Rt = 4, Ft = 256, Dt = 64, Ht = 63, nt = (int)std::max<size_t>(n / 8, 16);
        std::vector<float> xt((size_t)(nt + Ht) * Rt * Ft, 0.5f);
        std::vector<int32_t> tt((size_t)Dt * Ft);
        for (int d = 0; d < Dt; d++)
            for (int f = 0; f < Ft; f++) tt[(size_t)d * Ft + f] = d * (Ft - 1 - f) / (Ft - 1);
        auto dd = clDedisperser::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, Rt, Ft, Dt, Ht, tt);
        std::vector<float> y((size_t)nt * Rt * Dt, -1.0f);
        gr_vector_const_void_star in = {xt.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = dd->work(nt, in, out); });
        // 256 channels of a constant 1/2: every output is 128
        report("clDedisperser (4 x 256 x 64 trials, timing)", (size_t)nt, t, got == nt && y[0] == 128.0f && y[y.size() / 2] == 128.0f && y.back() == 128.0f);
    }
    return g_fail ? 1 : 0;
}

// --psearch-only: clPulseSearch at (R, D, K, Tb) = (2, 5, 4, 32), 3 blocks, on samples from the 32-bit linear congruential generator
// of --beamform-only (the top byte of each state as int8, as float: every boxcar sum is an exact integer), mean 0 and inv_sigma 1.
// Prints a "checksum" line that tests/test_psearch_gpu.py compares with the numpy reference: sum_i (i % 7 + 1) (loc_i + bits of
// snr_i) modulo 2^64 over the peak records in memory order; then one timing row.
static int psearch_test(size_t n)
{
    const int R = 2, D = 5, K = 4, Tb = 32, NB = 3, Hs = (1 << (K - 1)) - 1;
    uint32_t state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return (float)(int8_t)(state >> 24); };
    std::vector<float> x((size_t)(NB * Tb + Hs) * R * D);
    for (auto &v : x) v = next();
    {
        auto ps = clPulseSearch::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, R, D, K, Tb);
        bool ok = (int)ps->history() == Hs + 1 && ps->lookahead() == Hs && (int)ps->decimation() == Tb && ps->route().compare(0, 10, "tiled time") == 0 &&
                  ps->mean() == std::vector<float>((size_t)R * D, 0.0f) && ps->inv_sigma() == std::vector<float>((size_t)R * D, 1.0f);
        std::vector<clPulseSearch::peak> y((size_t)NB * R * D, clPulseSearch::peak{-1e30f, 0u});
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && ps->work(NB, in, out) == NB;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        unsigned long long sum = 0;
        for (size_t i = 0; i < y.size(); i++) {
            uint32_t bits;
            memcpy(&bits, &y[i].snr, 4);
            ok = ok && y[i].snr != -1e30f && (y[i].loc >> 24) < (uint32_t)K && (y[i].loc & 0xFFFFFFu) < (uint32_t)Tb;
            sum += (unsigned long long)(i % 7 + 1) * ((unsigned long long)y[i].loc + bits);
        }
        printf("clPulseSearch checksum %llu\n", sum);
        report("clPulseSearch (2 rows, 5 trials, 4 widths, blocks of 32)", (size_t)NB, dt.count(), ok);
    }
    {
        const int Rt = 4, Dt = 64, Kt = 8, Tbt = 256, Ht = (1 << (Kt - 1)) - 1, nb = (int)std::max<size_t>(n / 1024, 2);
        std::vector<float> xt((size_t)(nb * Tbt + Ht) * Rt * Dt, 0.5f);
        auto ps = clPulseSearch::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, Rt, Dt, Kt, Tbt);
        std::vector<clPulseSearch::peak> y((size_t)nb * Rt * Dt, clPulseSearch::peak{-1.0f, 0u});
        gr_vector_const_void_star in = {xt.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = ps->work(nb, in, out); });
        // a constant 1/2: snr_k = 2^(k/2) / 2 grows with k, so every peak is the widest boxcar at the block's first sample
        const uint32_t want = 7u << 24;
        report("clPulseSearch (4 x 64 series, 8 widths, timing)", (size_t)nb, t,
               got == nb && y[0].loc == want && y[y.size() / 2].loc == want && y.back().loc == want && y.back().snr > 5.6f && y.back().snr < 5.7f);
    }
    return g_fail ? 1 : 0;
}

// --fbclean-only: clFilterbankCleaner at (R, F, Tb) = (2, 256, 32), 3 blocks, zero-DM on, on samples from the 32-bit linear
// congruential generator of --beamform-only (the top byte of each state plus 1 as float: 1 .. 256, a power-like positive series) with
// channel 7 masked.  Prints a "checksum" line that tests/test_fbclean_gpu.py compares with the numpy reference: sum_i (i % 7 + 1)
// (bits of out_i) + sum_j (j % 5 + 1) tflag_j + sum_k (k % 3 + 1) cflag_k modulo 2^64, the channel flags taken once per block; then one
// timing row.
static int fbclean_test(size_t n)
{
    const int R = 2, F = 256, Tb = 32, NB = 3, N = NB * Tb;
    uint32_t state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return (float)(state >> 24) + 1.0f; };
    std::vector<float> x((size_t)N * R * F);
    for (auto &v : x) v = next();
    std::vector<uint8_t> mask((size_t)F, 0);
    mask[7] = 1;
    {
        auto fc = clFilterbankCleaner::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, R, F, Tb, 1.0, 0.0, 1.0, 4.0, true, mask);
        bool ok = (int)fc->history() == 1 && fc->output_multiple() == Tb && fc->block_len() == Tb && fc->route().compare(0, 5, "slab ") == 0 &&
                  fc->mask() == mask && fc->limits() == std::vector<double>{1.0, 0.0, 1.0, 4.0, 1.0};
        std::vector<float> y(x.size(), -1e30f);
        std::vector<uint8_t> tf((size_t)N * R, 0xEE), cf((size_t)N * R * F, 0xEE);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data(), tf.data(), cf.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && fc->work(N, in, out) == N;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        unsigned long long sum = 0;
        for (size_t i = 0; i < y.size(); i++) {
            uint32_t bits;
            memcpy(&bits, &y[i], 4);
            ok = ok && y[i] != -1e30f;
            sum += (unsigned long long)(i % 7 + 1) * bits;
        }
        for (size_t j = 0; j < tf.size(); j++) {
            ok = ok && tf[j] <= 1;
            sum += (unsigned long long)(j % 5 + 1) * tf[j];
        }
        const size_t cb = (size_t)R * F;
        for (size_t t = 0; t < (size_t)N; t++)  // every item of a block carries its block's flags
            ok = ok && memcmp(cf.data() + t * cb, cf.data() + (t / Tb) * Tb * cb, cb) == 0;
        for (size_t b = 0; b < (size_t)NB; b++)
            for (size_t k = 0; k < cb; k++) {
                const uint8_t c = cf[b * Tb * cb + k];
                ok = ok && c <= 1 && (k % F != 7 || c == 1);
                sum += (unsigned long long)((b * cb + k) % 3 + 1) * c;
            }
        printf("clFilterbankCleaner checksum %llu\n", sum);
        report("clFilterbankCleaner (2 rows, 256 channels, blocks of 32)", (size_t)N, dt.count(), ok);
    }
    {
        const int Rt = 4, Ft = 1024, Tbt = 256, nb = (int)std::max<size_t>(n / 4096, 2), nt = nb * Tbt;
        std::vector<float> xt((size_t)nt * Rt * Ft);
        for (size_t i = 0; i < xt.size(); i++) xt[i] = (i / ((size_t)Rt * Ft)) & 1 ? 3.0f : 1.0f;  // 1, 3, 1, 3 along time: m 2, var 1
        auto fc = clFilterbankCleaner::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, Rt, Ft, Tbt);
        std::vector<float> y(xt.size(), 0.0f);
        gr_vector_const_void_star in = {xt.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = fc->work(nt, in, out); });
        report("clFilterbankCleaner (4 x 1024 channels, blocks of 256, timing)", (size_t)nt, t,
               got == nt && y[0] == -1.0f && y[(size_t)Rt * Ft] == 1.0f && y.back() == 1.0f);
    }
    return g_fail ? 1 : 0;
}

// --fold-only: clFolder at (R, F, nbin, Ts) = (2, 256, 8, 32), 3 sub-integrations from T = 1000, on the samples of --fbclean-only, with the
// models {0, floor(2^64 / 9), 0} and {2^62, floor(2^64 / 5) + 3, -2^44}, through the optional hits output and the "models" port.  Prints a
// "checksum" line that tests/test_fold_gpu.py compares with the numpy reference: sum_i (i % 7 + 1) (bits of out_i) + sum_j (j % 5 + 1)
// hits_j modulo 2^64; then one timing row.
static int fold_test(size_t n)
{
    const int R = 2, F = 256, NBIN = 8, Ts = 32, NS = 3, N = NS * Ts;
    uint32_t state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return (float)(state >> 24) + 1.0f; };
    std::vector<float> x((size_t)N * R * F);
    for (auto &v : x) v = next();
    const std::vector<uint64_t> models = {0, UINT64_MAX / 9, 0, 1ull << 62, UINT64_MAX / 5 + 3, (uint64_t)-(1ll << 44)};
    {
        auto fo = clFolder::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, R, F, NBIN, Ts, std::vector<uint64_t>(6, 0));
        bool ok = (int)fo->history() == 1 && (int)fo->decimation() == Ts && fo->subint_len() == Ts && fo->nbin() == NBIN &&
                  fo->route().compare(0, 5, "bins ") == 0;
#ifndef MI355_WITH_GNURADIO
        ok = ok && fo->message_ports_in().size() == 1 && fo->message_ports_in()[0] == "models";
        ok = ok && fo->post_u64vector("models", models) && fo->models() == models;
        ok = ok && fo->post_u64vector("models", std::vector<uint64_t>(5, 1)) && fo->models() == models;  // a message of another size is dropped
#else
        fo->set_models(models);
#endif
        fo->set_sample(900);
        fo->skip(100);
        std::vector<float> y((size_t)NS * R * NBIN * F, -1e30f);
        std::vector<uint32_t> hits((size_t)NS * R * NBIN, 0xEEEEEEEEu);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data(), hits.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && fo->work(NS, in, out) == NS && fo->sample() == 1000u + N;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        unsigned long long sum = 0, total = 0;
        for (size_t i = 0; i < y.size(); i++) {
            uint32_t bits;
            memcpy(&bits, &y[i], 4);
            ok = ok && y[i] >= 0.0f;
            sum += (unsigned long long)(i % 7 + 1) * bits;
        }
        for (size_t j = 0; j < hits.size(); j++) {
            total += hits[j];
            sum += (unsigned long long)(j % 5 + 1) * hits[j];
        }
        ok = ok && total == (unsigned long long)N * R;
        printf("clFolder checksum %llu\n", sum);
        report("clFolder (2 rows, 256 channels, 8 bins, sub-integrations of 32)", (size_t)N, dt.count(), ok);
    }
    {
        const int Rt = 4, Ft = 1024, Bt = 4, Tst = 256, ns = (int)std::max<size_t>(n / 4096, 2), nt = ns * Tst;
        std::vector<float> xt((size_t)nt * Rt * Ft);
        for (size_t i = 0; i < xt.size(); i++) xt[i] = (float)((i / ((size_t)Rt * Ft)) & 3);  // 0, 1, 2, 3 along time
        std::vector<uint64_t> mt;
        for (int r = 0; r < Rt; r++) { mt.push_back(0); mt.push_back(1ull << 62); mt.push_back(0); }  // a period of four samples: bin = T mod 4
        auto fo = clFolder::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, Rt, Ft, Bt, Tst, mt);
        std::vector<float> y((size_t)ns * Rt * Bt * Ft, -1.0f);
        gr_vector_const_void_star in = {xt.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { fo->set_sample(0); got = fo->work(ns, in, out); });
        report("clFolder (4 x 1024 channels, 4 bins, sub-integrations of 256, timing)", (size_t)nt, t,
               got == ns && y[0] == 0.0f && y[(size_t)Ft] == 64.0f && y[(size_t)3 * Ft] == 192.0f && y.back() == 192.0f);
    }
    return g_fail ? 1 : 0;
}

// --ffa-only: clPeriodSearch at its smallest shape (S, p_lo..p_hi, L, K) = (1, 16..16, 1, 1) on the samples of --fbclean-only, with the
// optional profile output.  Prints a "checksum" line that tests/test_ffa_gpu.py compares with the numpy reference: sum_i (i % 7 + 1)
// (bits of snr_i) + sum_i (i % 7 + 1) loc_i + sum_j (j % 5 + 1) (bits of profile_j) modulo 2^64; then one timing row.
static int ffa_test(size_t n)
{
    {
        const int S = 1, P_LO = 16, P_HI = 16, L = 1, K = 1, M = 1 << L, N = M * P_HI;
        uint32_t state = 12345u;
        auto next = [&]() { state = state * 1664525u + 1013904223u; return (float)(state >> 24) + 1.0f; };
        std::vector<float> x((size_t)S * N);
        for (auto &v : x) v = next();
        auto fs = clPeriodSearch::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, S, P_LO, P_HI, L, K);
        bool ok = (int)fs->history() == 1 && fs->segment_len() == N && fs->records_per_series() == M && fs->route().compare(0, 6, "fused ") == 0 &&
                  fs->period(16, 1, 0.5) == 8.5;
        std::vector<clPeriodSearch::peak> y((size_t)S * M, clPeriodSearch::peak{-1e30f, 0u});
        std::vector<float> prof((size_t)S * M * P_HI, -1e30f);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data(), prof.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && fs->work(1, in, out) == 1;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        unsigned long long sum = 0;
        for (size_t i = 0; i < y.size(); i++) {
            uint32_t bits;
            memcpy(&bits, &y[i].snr, 4);
            ok = ok && y[i].snr != -1e30f && (y[i].loc >> 24) < (uint32_t)K && (y[i].loc & 0xFFFFFFu) < (uint32_t)P_HI;
            sum += (unsigned long long)(i % 7 + 1) * bits + (unsigned long long)(i % 7 + 1) * y[i].loc;
        }
        for (size_t j = 0; j < prof.size(); j++) {
            uint32_t bits;
            memcpy(&bits, &prof[j], 4);
            ok = ok && prof[j] >= 2.0f;
            sum += (unsigned long long)(j % 5 + 1) * bits;
        }
        printf("clPeriodSearch checksum %llu\n", sum);
        report("clPeriodSearch (1 series, base period 16, 2 rows, 1 width)", (size_t)N, dt.count(), ok);
    }
    {
        const int St = 16, Pt = 250, Lt = 8, Kt = 5, Nt = Pt << Lt;
        (void)n;
        std::vector<float> xt((size_t)St * Nt, 0.5f);
        auto fs = clPeriodSearch::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, St, Pt, Pt + 1, Lt, Kt);
        std::vector<float> xin((size_t)St * fs->segment_len(), 0.5f);
        std::vector<clPeriodSearch::peak> y((size_t)St * fs->records_per_series(), clPeriodSearch::peak{-1.0f, 0u});
        gr_vector_const_void_star in = {xin.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = fs->work(1, in, out); });
        // a constant 1/2: every profile bin is 2^(L-1), snr_k = 2^(L+k-1) c_(L+k) grows with k, so every peak is the widest boxcar at bin 0
        const uint32_t want = (uint32_t)(Kt - 1) << 24;
        report("clPeriodSearch (16 series, base periods 250..251, 256 rows, 5 widths, timing)", (size_t)fs->segment_len() * St, t,
               got == 1 && y[0].loc == want && y[y.size() / 2].loc == want && y.back().loc == want && y.back().snr == 32.0f);
    }
    return g_fail ? 1 : 0;
}

// --ssearch-only: clSpectralSearch at its smallest shape (S, n, H, Bb, k_lo) = (1, 256, 5, 16, 1) on the samples of --fbclean-only, with
// the optional spectrum output.  Prints a "checksum" line of the records, sum_i (i % 7 + 1) (bits of snr_i) + sum_i (i % 7 + 1) loc_i
// modulo 2^64 (tests/test_ssearch_gpu.py recomputes it from the spectrum the row prints beside it, "spectrum" = sum_j (j % 5 + 1) (bits of
// w_j): the spectrum stage is floating point, the sums over it are exact); then one timing row.
static int ssearch_test(size_t n)
{
    {
        const int S = 1, N = 256, H = 5, BB = 16, K_LO = 1, NB = N / 2;
        uint32_t state = 12345u;
        auto next = [&]() { state = state * 1664525u + 1013904223u; return (float)(state >> 24) + 1.0f; };
        std::vector<float> x((size_t)S * N);
        for (auto &v : x) v = next();
        auto ss = clSpectralSearch::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, S, N, H, BB, K_LO, std::vector<float>(1, 1.0f / 64.0f));
        bool ok = (int)ss->history() == 1 && ss->segment_len() == N && ss->num_bins() == NB && ss->records_per_series() == NB / BB &&
                  ss->route().compare(0, 6, "tiled ") == 0 && ss->freq(2, 64, 0.5) == 0.125;
        std::vector<clSpectralSearch::peak> y((size_t)S * NB / BB, clSpectralSearch::peak{-1e30f, 0u});
        std::vector<float> w((size_t)S * NB, -1e30f);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data(), w.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && ss->work(1, in, out) == 1;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        unsigned long long sum = 0, wsum = 0;
        for (size_t i = 0; i < y.size(); i++) {
            uint32_t bits;
            memcpy(&bits, &y[i].snr, 4);
            ok = ok && y[i].snr != -1e30f && (y[i].loc >> 24) <= (uint32_t)H && (y[i].loc & 0xFFFFFFu) < (uint32_t)BB;
            sum += (unsigned long long)(i % 7 + 1) * bits + (unsigned long long)(i % 7 + 1) * y[i].loc;
        }
        for (size_t j = 0; j < w.size(); j++) {
            uint32_t bits;
            memcpy(&bits, &w[j], 4);
            ok = ok && w[j] >= 0.0f;
            wsum += (unsigned long long)(j % 5 + 1) * bits;
        }
        printf("clSpectralSearch checksum %llu spectrum %llu\n", sum, wsum);
        for (size_t j = 0; j < w.size(); j++) {
            uint32_t bits;
            memcpy(&bits, &w[j], 4);
            printf("%s%08x", j % 16 ? " " : "w ", bits);
            if (j % 16 == 15) printf("\n");
        }
        report("clSpectralSearch (1 series, 256 samples, 5 folds, blocks of 16 bins)", (size_t)N, dt.count(), ok);
    }
    {
        const int St = 16, Nt = 1 << 16, Ht = 4, Bt = 256;
        (void)n;
        std::vector<float> xt((size_t)St * Nt, 0.0f);
        for (int s = 0; s < St; s++)
            for (int t = 0; t < Nt; t += 16) xt[(size_t)s * Nt + t] = 1.0f;  // a train of period 16: the spectrum is zero but for the multiples of bin 4096
        auto ss = clSpectralSearch::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, St, Nt, Ht, Bt, 1);
        std::vector<clSpectralSearch::peak> y((size_t)St * ss->records_per_series(), clSpectralSearch::peak{-1.0f, 0u});
        gr_vector_const_void_star in = {xt.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = ss->work(1, in, out); });
        // the seven harmonics 4096 m, m = 1 .. 7, hold 4096^2 / 65536 = 256 each: level 2 at bin 16384 = block 64 sums four of them,
        // snr = (1024 - 4) / 2 = 510, the largest of the series
        bool ok = got == 1;
        for (int s = 0; s < St; s++) {
            float best = -1.0f;
            size_t at = 0;
            for (size_t b = 0; b < (size_t)ss->records_per_series(); b++)
                if (y[(size_t)s * ss->records_per_series() + b].snr > best) { best = y[(size_t)s * ss->records_per_series() + b].snr; at = b; }
            ok = ok && at == 64 && best > 509.99f && best < 510.01f && y[(size_t)s * ss->records_per_series() + at].loc == (2u << 24);
        }
        report("clSpectralSearch (16 series, 65536 samples, 4 folds, blocks of 256 bins, timing)", (size_t)Nt * St, t, ok);
    }
    return g_fail ? 1 : 0;
}

// --accel-only: clAccelResampler at (S, n, A) = (2, 4099, 3) -- an odd length, so the 4-byte head and tail stores run -- with the trials
// {0, 2^63 / n, -apex}, apex the smallest c whose shift at mid-series reaches 2, on the 32-bit words of the generator of --fbclean-only.
// Prints a "checksum" line of the output, sum_j (j % 7 + 1) word_j modulo 2^64 (tests/test_accel_gpu.py recomputes it from
// tests/accel_ref.py); then one timing row.
static int accel_test(size_t n)
{
    {
        const int S = 2, N = 4099;
        uint32_t state = 12345u;
        std::vector<uint32_t> x((size_t)S * N);
        for (auto &v : x) { state = state * 1664525u + 1013904223u; v = state; }
        const long long top = (long long)((1ull << 63) / (unsigned)N);
        const unsigned __int128 dmax = (unsigned __int128)(N / 2) * (unsigned)(N - N / 2);
        const long long apex = (long long)((((unsigned __int128)3 << 63) + dmax - 1) / dmax);
        const std::vector<long long> trials = {0, top, -apex};
        auto ar = clAccelResampler::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, S, N, trials);
        bool ok = (int)ar->history() == 1 && ar->segment_len() == N && ar->num_trials() == 3 && ar->rows() == 6 &&
                  ar->route().compare(0, 6, "tiled ") == 0 && ar->trials() == trials;
        std::vector<uint32_t> y((size_t)S * 3 * N, 0xFFFFFFFFu);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data()};
        auto t0 = std::chrono::steady_clock::now();
        ok = ok && ar->work(1, in, out) == 1;
        std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
        unsigned long long sum = 0;
        for (size_t j = 0; j < y.size(); j++) sum += (unsigned long long)(j % 7 + 1) * y[j];
        for (int s = 0; s < S; s++) {
            ok = ok && !memcmp(&y[(size_t)s * 3 * N], &x[(size_t)s * N], (size_t)N * 4);  // c = 0 is the identity
            for (int t = 0; t < 3; t++)  // the end points stay
                ok = ok && y[((size_t)s * 3 + t) * N] == x[(size_t)s * N] && y[((size_t)s * 3 + t) * N + N - 1] == x[(size_t)s * N + N - 1];
        }
        printf("clAccelResampler checksum %llu\n", sum);
        report("clAccelResampler (2 series, 4099 samples, 3 trials)", (size_t)N, dt.count(), ok);
    }
    {
        const int St = 16, Nt = 1 << 16, At = 8;
        (void)n;
        std::vector<float> xt((size_t)St * Nt);
        for (size_t i = 0; i < xt.size(); i++) xt[i] = (float)(i % (size_t)Nt);  // a ramp: an output sample is its own source index
        const long long step = (long long)(((unsigned __int128)1 << 66) / ((unsigned __int128)Nt * Nt));  // one sample at mid-series
        std::vector<long long> ladder;
        for (int j = -4; j < 4; j++) ladder.push_back(j * step);
        auto ar = clAccelResampler::make(OCLTYPE_GPU, OCLDEVICESELECTOR_SPECIFIC, 0, g_dev, St, Nt, ladder);
        std::vector<float> y((size_t)St * At * Nt, -1.0f);
        gr_vector_const_void_star in = {xt.data()};
        gr_vector_void_star out = {y.data()};
        int got = 0;
        const double t = time_calls([&] { got = ar->work(1, in, out); });
        // trial j shifts the middle sample by j and leaves the ends; the sources never decrease
        bool ok = got == 1;
        for (int s = 0; s < St; s++)
            for (int a = 0; a < At; a++) {
                const float *r = &y[((size_t)s * At + a) * Nt];
                ok = ok && r[0] == 0.0f && r[Nt - 1] == (float)(Nt - 1) && r[Nt / 2] == (float)(Nt / 2 + a - 4);
                for (int i = 1; i < Nt && ok; i++) ok = r[i] >= r[i - 1];
            }
        report("clAccelResampler (16 series, 65536 samples, 8 trials, timing)", (size_t)Nt * St, t, ok);
    }
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv)
{
    size_t n = 8192;  // the reference's default block size
    int fft_size = 4096, ntaps = 65;
    bool only_fft = false, only_xcorrelate = false, xc_complex = false, only_loops = false, only_resampler = false, only_synth = false, only_pspec = false, only_xlate = false, only_beamform = false, only_fengine = false, only_dedisp = false, only_psearch = false, only_fbclean = false, only_fold = false, only_ffa = false, only_ssearch = false, only_accel = false;
    int xc_inputs = 2, xc_maxsearch = 512;
    for (int i = 1; i < argc; i++) {
        if (!strncmp(argv[i], "--device=", 9)) g_dev = atoi(argv[i] + 9);
        else if (!strncmp(argv[i], "--iterations=", 13)) g_iter = atoi(argv[i] + 13);
        else if (!strcmp(argv[i], "--iterations") && i + 1 < argc) g_iter = atoi(argv[++i]);
        else if (!strncmp(argv[i], "--fft-size=", 11)) fft_size = atoi(argv[i] + 11);
        else if (!strncmp(argv[i], "--ntaps=", 8)) ntaps = atoi(argv[i] + 8);
        else if (!strcmp(argv[i], "--fft-only")) only_fft = true;
        else if (!strcmp(argv[i], "--xcorrelate-only")) only_xcorrelate = true;
        else if (!strcmp(argv[i], "--loops-only")) only_loops = true;
        else if (!strcmp(argv[i], "--resampler-only")) only_resampler = true;
        else if (!strcmp(argv[i], "--synth-only")) only_synth = true;
        else if (!strcmp(argv[i], "--pspec-only")) only_pspec = true;
        else if (!strcmp(argv[i], "--xlate-only")) only_xlate = true;
        else if (!strcmp(argv[i], "--beamform-only")) only_beamform = true;
        else if (!strcmp(argv[i], "--fengine-only")) only_fengine = true;
        else if (!strcmp(argv[i], "--dedisp-only")) only_dedisp = true;
        else if (!strcmp(argv[i], "--psearch-only")) only_psearch = true;
        else if (!strcmp(argv[i], "--fbclean-only")) only_fbclean = true;
        else if (!strcmp(argv[i], "--fold-only")) only_fold = true;
        else if (!strcmp(argv[i], "--ffa-only")) only_ffa = true;
        else if (!strcmp(argv[i], "--ssearch-only")) only_ssearch = true;
        else if (!strcmp(argv[i], "--accel-only")) only_accel = true;
        else if (!strncmp(argv[i], "--num_inputs=", 13)) xc_inputs = atoi(argv[i] + 13);
        else if (!strncmp(argv[i], "--maxsearch=", 12)) xc_maxsearch = atoi(argv[i] + 12);
        else if (!strcmp(argv[i], "--input_complex")) xc_complex = true;
        else if (!strncmp(argv[i], "--xengine-stream=", 17)) {
            try { return xengine_stream_test(argv[i] + 17); }
            catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
        }
        else if (!strcmp(argv[i], "--scheduler-contract")) {
            try { return scheduler_contract_test(); }
            catch (const std::exception &e) { fprintf(stderr, "scheduler contract test: %s\n", e.what()); return 2; }
        }
        else if (!strncmp(argv[i], "--xengine-e2e", 13)) {
            try { return xengine_e2e(argv[i][13] == '=' ? atoi(argv[i] + 14) : 5); }
            catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
        }
        else if (!strcmp(argv[i], "--help")) {
            printf("usage: %s [--device=N] [--iterations=N] [--fft-size=N] [--ntaps=N] [--fft-only] [block size]\n"
                   "       %s --xcorrelate-only [--num_inputs=N] [--maxsearch=N] [--input_complex] [--iterations=N] [signal length]\n"
                   "       %s --loops-only [--iterations=N] [block size]\n"
                   "       %s --resampler-only [--iterations=N] [block size]\n"
                   "       %s --synth-only [--iterations N] [block size]\n"
                   "       %s --pspec-only [--iterations N] [block size]\n"
                   "       %s --xlate-only [--iterations N] [block size]\n"
                   "       %s --beamform-only [--iterations N] [block size]\n"
                   "       %s --fengine-only [--iterations N] [block size]\n"
                   "       %s --dedisp-only [--iterations N] [block size]\n"
                   "       %s --psearch-only [--iterations N] [block size]\n"
                   "       %s --fbclean-only [--iterations N] [block size]\n"
                   "       %s --fold-only [--iterations N] [block size]\n"
                   "       %s --ffa-only [--iterations N]\n"
                   "       %s --ssearch-only [--iterations N]\n"
                   "       %s --accel-only [--iterations N]\n",
                   argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
            return 0;
        } else n = strtoull(argv[i], nullptr, 10);
    }
    if (only_loops) {
        try { return loops_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_resampler) {
        try { return resampler_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_synth) {
        try { return synth_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_pspec) {
        try { return pspec_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_xlate) {
        try { return xlate_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_beamform) {
        try { return beamform_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_fengine) {
        try { return fengine_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_dedisp) {
        try { return dedisp_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_psearch) {
        try { return psearch_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_fbclean) {
        try { return fbclean_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_fold) {
        try { return fold_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_ffa) {
        try { return ffa_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_ssearch) {
        try { return ssearch_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_accel) {
        try { return accel_test(n); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    if (only_xcorrelate) {
        try { return xcorrelate_test(n, xc_inputs, xc_maxsearch, xc_complex); }
        catch (const std::exception &e) { std::cerr << "error: " << e.what() << std::endl; return 2; }
    }
    try {
        printf("test-clenabled-mi355: block size %zu, %d iterations, device %d (times include H2D + D2H)\n", n, g_iter, g_dev);
        if (!only_fft) test_math(n);
        test_fft(fft_size, std::max<size_t>(n, fft_size));
        if (!only_fft) {
            test_filter(ntaps, std::max<size_t>(n, 32768));
            test_pfb();
            test_xengine(16, 256, 256);
            test_elem(n);
            test_xcorr(std::min(fft_size, 4096), std::max<size_t>(n, fft_size));
        }
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 2;
    }
    return g_fail ? 1 : 0;
}
