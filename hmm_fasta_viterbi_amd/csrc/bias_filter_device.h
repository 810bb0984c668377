// bias_filter_device.h -- what the cascade (fwd_device.cpp, msv_fwd_filter_batch_opts) needs of a bias-filter
// profile beyond msv.h: the profile's own buffers for the bias of a batch and the filtered survivor list.
#pragma once

#include <cstdint>

#include "msv.h"

namespace bfdev {

// Room for n sequences: *d_bias float [n], *d_sel uint32 [n], *d_count one device word.  The profile's device must
// be current.
msv_status cascade_buffers(msv_bf_profile* p, uint64_t n, float** d_bias, uint32_t** d_sel, uint32_t** d_count);
int device_of(const msv_bf_profile* p);

}  // namespace bfdev
