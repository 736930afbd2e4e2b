// host_lzp.hpp — unlzp on a host core (host_lzp.cpp)
//
// The same bytes, length and ok / failed verdict as k_lzp_dec (lzp.hip): a
// stream of literals and of match tokens whose source is the last position
// with the same hash of the 4 bytes before it.  The chain is serial whoever
// runs it: the kernel steps it with one wave, a table in global memory and a
// fence per marker byte; a host core keeps the 256 KB table in its cache.  The
// name sections' comment streams (names.cpp) decode here, since their output
// is wanted on the host anyway.  No HIP in this file or its .cpp.
#pragma once
#include <cstddef>
#include <cstdint>

namespace fqz5 {
namespace host {

// in[0, in_len) into out[0, cap): *out_len the bytes written.  False (the
// kernel's status -1): the output would pass cap, or a marker's length
// byte(s) or its escaped literal lie past in_len; *out_len is then what was
// written before the failing token.  Reads stay inside [in, in + in_len),
// writes inside [out, out + cap).  The 65536-entry table is the call's own.
bool unlzp(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap, size_t *out_len);

}  // namespace host
}  // namespace fqz5
