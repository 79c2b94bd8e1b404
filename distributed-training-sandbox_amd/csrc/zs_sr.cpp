// Host entry points of the stochastic-rounding generator (csrc/zs_sr.h): the definition the kernels
// use, for callers and tests that restate it.  Plain C++, no device is touched.
#include "zs_common.h"
#include "zs_sr.h"

extern "C" {

int zs_sr_keys(uint64_t seed, uint64_t step, uint32_t* key0, uint32_t* key1) {
  ZS_REQUIRE(key0 && key1, "zs_sr_keys: NULL argument");
  zs_sr::keys(seed, step, key0, key1);
  return ZS_OK;
}

int zs_sr_bits(uint64_t e, uint32_t key0, uint32_t key1, uint32_t* r) {
  ZS_REQUIRE(r != nullptr, "zs_sr_bits: NULL argument");
  *r = zs_sr::bits(e, key0, key1);
  return ZS_OK;
}

int zs_sr_pkeys(uint32_t key0, uint32_t key1, uint32_t* pkey0, uint32_t* pkey1) {
  ZS_REQUIRE(pkey0 && pkey1, "zs_sr_pkeys: NULL argument");
  zs_sr::pkeys(key0, key1, pkey0, pkey1);
  return ZS_OK;
}

}  // extern "C"
