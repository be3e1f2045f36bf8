// pcppx_args.h — the argument rules that the message operators' valid_args (pcppx_tlsfp.h, pcppx_dns.h, pcppx_http.h,
// pcppx_ssl.h, pcppx_dhcp.h; sip delegates to http) begin and end with. Plain C++ without HIP: the *_ref.cpp files
// compile it with a host compiler alone.
#pragma once

#include <stdint.h>

#include "pcppx.h"

namespace pcppx
{
// b and r are there; max_layers in range over FIXED rows; with packets, the records and the batch's arrays are there
// (data may be null only with data_len 0).
inline bool valid_source(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers)
{
	if (b == nullptr || r == nullptr)
		return false;
	if (max_layers == 0 || max_layers > PCPPX_MAX_LAYERS || r->layout != PCPPX_LAYOUT_FIXED)
		return false;
	if (b->n != 0 && (r->layers == nullptr || (r->summary == nullptr && r->brief == nullptr)))
		return false;
	return b->n == 0 || (b->offsets != nullptr && b->caplens != nullptr && (b->data != nullptr || b->data_len == 0));
}
}  // namespace pcppx
