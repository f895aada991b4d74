// Scheduler-facing base classes of the block layer.
//
// With GNU Radio installed (CMake finds it and defines MI355_WITH_GNURADIO) these are GNU Radio's own gr::block /
// gr::sync_block / gr::sync_decimator, gr::io_signature, message ports (pmt) and stream tags, and the blocks of
// lib/clenabled_impl.cc are ordinary out-of-tree blocks.  This image has no GNU Radio, so the same block code also compiles
// against the small stand-alone classes below: the same constructor shape (name, input signature, output signature), the
// same calls (set_history, set_output_multiple, consume / consume_each, message_port_register_out) -- they RECORD what the
// block asked of the scheduler so that the CLI and the tests can act as the scheduler and check it.  Nothing here computes.
#pragma once
#ifdef MI355_WITH_GNURADIO
#include <gnuradio/block.h>
#include <gnuradio/io_signature.h>
#include <gnuradio/logger.h>
#include <gnuradio/sptr_magic.h>
#include <gnuradio/sync_block.h>
#include <gnuradio/sync_decimator.h>
#include <pmt/pmt.h>
#include <functional>
#include <vector>
#else
#include <complex>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
typedef std::complex<float> gr_complex;
typedef std::vector<int> gr_vector_int;
typedef std::vector<const void *> gr_vector_const_void_star;
typedef std::vector<void *> gr_vector_void_star;
namespace gr {
class io_signature {
    int d_min, d_max;
    std::vector<int> d_sizes;
public:
    typedef std::shared_ptr<io_signature> sptr;
    static constexpr int IO_INFINITE = -1;
    io_signature(int mn, int mx, const std::vector<int> &sizes) : d_min(mn), d_max(mx), d_sizes(sizes) {}
    static sptr make(int min_streams, int max_streams, int sizeof_stream_item)
    {
        return std::make_shared<io_signature>(min_streams, max_streams, std::vector<int>{sizeof_stream_item});
    }
    static sptr makev(int min_streams, int max_streams, const std::vector<int> &sizes)
    {
        return std::make_shared<io_signature>(min_streams, max_streams, sizes);
    }
    int min_streams() const { return d_min; }
    int max_streams() const { return d_max; }
    int sizeof_stream_item(int i) const { return d_sizes.empty() ? 0 : d_sizes[(size_t)i < d_sizes.size() ? i : d_sizes.size() - 1]; }
};

// one published message of the stand-alone build: port, key of the pair, and either a complex vector or an integer;
// clXCorrelate's PDU (a dict of "corrvect" f32vector and "corrective_lags" s32vector) is one message with key "corrvect" and both
struct shim_message {
    std::string port, key;
    std::vector<gr_complex> c32;
    uint64_t u64 = 0;
    std::vector<float> f32;
    std::vector<int32_t> s32;
};

class basic_block_shim {
    std::string d_name;
    io_signature::sptr d_in, d_out;
    unsigned d_history = 1;
    int d_output_multiple = 1;
    uint64_t d_rate_interp = 1, d_rate_decim = 1;
    std::vector<long> d_consumed;  // per input, since the last reset_consumed()
    std::vector<long> d_offered, d_offer_base;  // set_offered(): what the caller acting as scheduler offers the next general_work()
    std::vector<std::string> d_out_ports, d_in_ports;
    std::map<std::string, std::function<void(double)>> d_in_handlers;
    std::map<std::string, std::function<void(const std::vector<uint64_t> &)>> d_in_u64_handlers;
    std::deque<shim_message> d_messages;
    std::vector<uint64_t> d_first_tags;  // what get_tags_in_window(i, 0, 1) would return, set by the caller acting as scheduler

protected:
    basic_block_shim() {}  // (interface classes; the _impl constructs the virtual base)

public:
    basic_block_shim(const std::string &name, io_signature::sptr in, io_signature::sptr out) : d_name(name), d_in(in), d_out(out) {}
    virtual ~basic_block_shim() {}
    const std::string &name() const { return d_name; }
    io_signature::sptr input_signature() const { return d_in; }
    io_signature::sptr output_signature() const { return d_out; }
    unsigned history() const { return d_history; }
    void set_history(unsigned h) { d_history = h; }
    int output_multiple() const { return d_output_multiple; }
    void set_output_multiple(int m) { d_output_multiple = m; }
    void set_relative_rate(uint64_t interpolation, uint64_t decimation) { d_rate_interp = interpolation; d_rate_decim = decimation; }
    uint64_t relative_rate_i() const { return d_rate_interp; }
    uint64_t relative_rate_d() const { return d_rate_decim; }
    virtual bool start() { return true; }
    virtual bool stop() { return true; }
    // general_work() side of the contract
    void consume(int which_input, int how_many)
    {
        if ((size_t)which_input >= d_consumed.size()) d_consumed.resize(which_input + 1, 0);
        d_consumed[which_input] += how_many;
        // GNU Radio's read pointer must not pass its write pointer: a block never consumes more than it was offered
        if ((size_t)which_input < d_offered.size() && d_consumed[which_input] - d_offer_base[which_input] > d_offered[which_input])
            throw std::logic_error(d_name + ": consume() of more items than general_work() was offered");
    }
    void consume_each(int how_many)
    {
        const int n = d_in ? (d_in->max_streams() > 0 ? d_in->max_streams() : (int)d_consumed.size()) : 1;
        for (int i = 0; i < (n > 0 ? n : 1); i++) consume(i, how_many);
    }
    long nitems_consumed(int which_input) const { return (size_t)which_input < d_consumed.size() ? d_consumed[which_input] : 0; }
    void reset_consumed()
    {
        d_consumed.assign(d_consumed.size(), 0);
        d_offered.clear();
        d_offer_base.clear();
    }
    // the items offered per input to the general_work() call that follows (ninput_items); consuming more than that throws
    void set_offered(const std::vector<int> &ninput_items)
    {
        d_offered.assign(ninput_items.begin(), ninput_items.end());
        d_offer_base.assign(ninput_items.size(), 0);
        for (size_t i = 0; i < d_offer_base.size() && i < d_consumed.size(); i++) d_offer_base[i] = d_consumed[i];
    }
    // message ports
    void message_port_register_out(const std::string &port) { d_out_ports.push_back(port); }
    const std::vector<std::string> &message_ports_out() const { return d_out_ports; }
    void shim_publish(shim_message &&m) { d_messages.push_back(std::move(m)); }
    bool pop_message(shim_message &m)
    {
        if (d_messages.empty()) return false;
        m = std::move(d_messages.front());
        d_messages.pop_front();
        return true;
    }
    // input message ports that carry one real number (cons(key, double) under GNU Radio): the block registers a handler, the caller
    // acting as scheduler delivers a value; false: no such port
    void message_port_register_in(const std::string &port) { d_in_ports.push_back(port); }
    const std::vector<std::string> &message_ports_in() const { return d_in_ports; }
    void set_double_handler(const std::string &port, std::function<void(double)> fn) { d_in_handlers[port] = std::move(fn); }
    bool post_double(const std::string &port, double value)
    {
        auto it = d_in_handlers.find(port);
        if (it == d_in_handlers.end()) return false;
        it->second(value);
        return true;
    }
    // input message ports that carry a vector of 64-bit words (cons(key, u64vector) under GNU Radio), delivered the same way
    void set_u64vector_handler(const std::string &port, std::function<void(const std::vector<uint64_t> &)> fn) { d_in_u64_handlers[port] = std::move(fn); }
    bool post_u64vector(const std::string &port, const std::vector<uint64_t> &value)
    {
        auto it = d_in_u64_handlers.find(port);
        if (it == d_in_u64_handlers.end()) return false;
        it->second(value);
        return true;
    }
    // stream tags: the first tag value of every input in the current window (set by the caller acting as scheduler)
    void set_first_tags(const std::vector<uint64_t> &t) { d_first_tags = t; }

protected:
    // reading tags is a protected service of gr::block (get_tags_in_window): only the block itself may ask
    bool shim_first_tag(int which_input, uint64_t &value) const
    {
        if ((size_t)which_input >= d_first_tags.size()) return false;
        value = d_first_tags[which_input];
        return true;
    }
};
class sync_block : public basic_block_shim {
protected:
    sync_block() {}
public:
    using basic_block_shim::basic_block_shim;
    virtual int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items) = 0;
};
class sync_decimator : public sync_block {
    unsigned d_decimation = 1;
protected:
    sync_decimator() {}
public:
    sync_decimator(const std::string &name, io_signature::sptr in, io_signature::sptr out, unsigned decimation)
        : sync_block(name, in, out), d_decimation(decimation) {}
    unsigned decimation() const { return d_decimation; }
};
class block : public basic_block_shim {
protected:
    block() {}
public:
    using basic_block_shim::basic_block_shim;
    virtual void forecast(int noutput_items, gr_vector_int &ninput_items_required) = 0;
    virtual int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &input_items,
                             gr_vector_void_star &output_items) = 0;
};
}  // namespace gr
#endif

// ---- the few scheduler services the blocks use, spelled once for both builds ------------------------------------
namespace gr {
namespace clenabled {
namespace sched {
#ifdef MI355_WITH_GNURADIO
inline void register_out(gr::basic_block *b, const char *port) { b->message_port_register_out(pmt::mp(port)); }
// message_port_pub(port, cons(intern(key), c32vector)) -- lib/clXEngine_impl.cc:1076-1077
inline void publish_c32vector(gr::basic_block *b, const char *port, const char *key, const gr_complex *v, size_t n)
{
    b->message_port_pub(pmt::mp(port), pmt::cons(pmt::string_to_symbol(key), pmt::init_c32vector(n, v)));
}
// message_port_pub(port, cons(intern(key), uint64)) -- lib/clXEngine_impl.cc:1203-1204
inline void publish_u64(gr::basic_block *b, const char *port, const char *key, uint64_t value)
{
    b->message_port_pub(pmt::mp(port), pmt::cons(pmt::intern(key), pmt::from_uint64(value)));
}
// clXCorrelate's PDU: cons(dict{"corrvect": f32vector, "corrective_lags": s32vector}, PMT_NIL) -- lib/clXCorrelate_impl.cc:1594-1600
inline void publish_corr_pdu(gr::basic_block *b, const char *port, const std::vector<float> &corr, const std::vector<int32_t> &lags)
{
    pmt::pmt_t meta = pmt::make_dict();
    meta = pmt::dict_add(meta, pmt::mp("corrvect"), pmt::init_f32vector(corr.size(), corr.data()));
    meta = pmt::dict_add(meta, pmt::mp("corrective_lags"), pmt::init_s32vector(lags.size(), lags.data()));
    b->message_port_pub(pmt::mp(port), pmt::cons(meta, pmt::PMT_NIL));
}
// input ports that carry cons(key, real) / cons(key, u64vector): a message that is no pair, or whose cdr is of another type, is dropped
// (the scheduler's thread has nobody to throw to)
inline void register_in_double(gr::basic_block *b, const char *port, std::function<void(double)> fn)
{
    b->message_port_register_in(pmt::mp(port));
    b->set_msg_handler(pmt::mp(port), [fn](pmt::pmt_t msg) {
        if (!pmt::is_pair(msg)) return;
        const pmt::pmt_t v = pmt::cdr(msg);
        if (pmt::is_real(v)) fn(pmt::to_double(v));
    });
}
inline void register_in_u64vector(gr::basic_block *b, const char *port, std::function<void(const std::vector<uint64_t> &)> fn)
{
    b->message_port_register_in(pmt::mp(port));
    b->set_msg_handler(pmt::mp(port), [fn](pmt::pmt_t msg) {
        if (!pmt::is_pair(msg)) return;
        const pmt::pmt_t v = pmt::cdr(msg);
        if (pmt::is_u64vector(v)) fn(pmt::u64vector_elements(v));
    });
}
// (reading the first tag of an input, get_tags_in_window, is protected in gr::block: a member of clXEngine_impl does it)
// blocks are handed to the scheduler through GNU Radio's initial-sptr registry, as every make() of the reference does
template <class T> std::shared_ptr<T> adopt(T *p) { return gnuradio::get_initial_sptr(p); }
inline void no_tag_propagation(gr::block *b) { b->set_tag_propagation_policy(gr::block::TPP_DONT); }
#else
inline void register_out(gr::basic_block_shim *b, const char *port) { b->message_port_register_out(port); }
inline void publish_c32vector(gr::basic_block_shim *b, const char *port, const char *key, const gr_complex *v, size_t n)
{
    gr::shim_message m;
    m.port = port;
    m.key = key;
    m.c32.assign(v, v + n);
    b->shim_publish(std::move(m));
}
inline void publish_u64(gr::basic_block_shim *b, const char *port, const char *key, uint64_t value)
{
    gr::shim_message m;
    m.port = port;
    m.key = key;
    m.u64 = value;
    b->shim_publish(std::move(m));
}
// (one message with key "corrvect" and both vectors, see shim_message)
inline void publish_corr_pdu(gr::basic_block_shim *b, const char *port, const std::vector<float> &corr, const std::vector<int32_t> &lags)
{
    gr::shim_message m;
    m.port = port;
    m.key = "corrvect";
    m.f32 = corr;
    m.s32 = lags;
    b->shim_publish(std::move(m));
}
inline void register_in_double(gr::basic_block_shim *b, const char *port, std::function<void(double)> fn)
{
    b->message_port_register_in(port);
    b->set_double_handler(port, std::move(fn));
}
inline void register_in_u64vector(gr::basic_block_shim *b, const char *port, std::function<void(const std::vector<uint64_t> &)> fn)
{
    b->message_port_register_in(port);
    b->set_u64vector_handler(port, std::move(fn));
}
template <class T> std::shared_ptr<T> adopt(T *p) { return std::shared_ptr<T>(p); }
inline void no_tag_propagation(gr::basic_block_shim *) {}
#endif
}  // namespace sched
}  // namespace clenabled
}  // namespace gr
