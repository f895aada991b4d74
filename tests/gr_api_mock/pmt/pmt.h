#pragma once
#include <complex>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
namespace pmt {
class pmt_base;
typedef std::shared_ptr<pmt_base> pmt_t;
pmt_t mp(const char *s);
pmt_t mp(const std::string &s);
pmt_t intern(const std::string &s);
pmt_t string_to_symbol(const std::string &s);
pmt_t cons(const pmt_t &x, const pmt_t &y);
pmt_t from_uint64(uint64_t x);
uint64_t to_uint64(pmt_t x);
pmt_t from_double(double x);
pmt_t init_c32vector(size_t k, const std::complex<float> *data);
pmt_t get_PMT_NIL();
#define PMT_NIL get_PMT_NIL()
bool is_pair(const pmt_t &obj);
pmt_t cdr(const pmt_t &pair);
bool is_real(pmt_t obj);
double to_double(pmt_t x);
bool is_u64vector(pmt_t x);
const std::vector<uint64_t> u64vector_elements(pmt_t v);
pmt_t make_dict();
pmt_t dict_add(const pmt_t &dict, const pmt_t &key, const pmt_t &value);
pmt_t init_f32vector(size_t k, const float *data);
pmt_t init_s32vector(size_t k, const int32_t *data);
}  // namespace pmt
