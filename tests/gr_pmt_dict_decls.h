// Declarations of the GNU Radio 3.10 pmt calls the clXCorrelate PDU needs (gnuradio-runtime include/pmt/pmt.h) and that
// tests/gr_api_mock/pmt/pmt.h does not carry; force-included by tests/test_xcorr_td.py.
#pragma once
#include <pmt/pmt.h>
namespace pmt {
pmt_t make_dict();
pmt_t dict_add(const pmt_t &dict, const pmt_t &key, const pmt_t &value);
pmt_t init_f32vector(size_t k, const float *data);
pmt_t init_s32vector(size_t k, const int32_t *data);
pmt_t get_PMT_NIL();
#define PMT_NIL get_PMT_NIL()
}  // namespace pmt
