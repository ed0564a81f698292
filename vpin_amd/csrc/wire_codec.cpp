// wire_codec.cpp -- the 24-byte frame header of the inference stream, encoded and decoded (include/vpin_hip.h has the layout and
// the table of types).  Plain C++: the bytes come from an untrusted peer, and tools/wire_check runs this file under the host
// compiler's sanitizers.  decode names the rule it rejects a header by; a receiver allocates only after it has accepted one.
#include <cstdio>
#include <cstring>

#include "wire.h"

namespace vpin::wire {

int fail(int code, const char* text) {
  set_error(text);
  return code;
}

namespace {

const uint8_t kMagic[4] = {'V', 'P', 'W', '1'};

void put_le(uint8_t* p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}
uint64_t get_le(const uint8_t* p, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

// the rules both directions share; who: the entry point the text names
int check(const vpin_wire_header& h, const char* who) {
  char why[160];
  if (h.type < VPIN_WIRE_HELLO || h.type > VPIN_WIRE_ERROR) {
    snprintf(why, sizeof why, "%s: unknown type %u", who, (unsigned)h.type);
    return fail(VPIN_EINVAL, why);
  }
  if (h.cnt > VPIN_WIRE_MAX_CNT) {
    snprintf(why, sizeof why, "%s: cnt %u is above VPIN_WIRE_MAX_CNT", who, (unsigned)h.cnt);
    return fail(VPIN_EINVAL, why);
  }
  bool ok = false;
  const uint64_t pts = 64 * (uint64_t)h.cnt;
  switch (h.type) {
    case VPIN_WIRE_HELLO: ok = h.cnt == 1 && h.payload_len == 32; break;
    case VPIN_WIRE_INPUT:
    case VPIN_WIRE_ROUND: ok = h.cnt >= 1 && h.payload_len == pts; break;
    case VPIN_WIRE_REPLY: ok = h.payload_len == pts; break;
    case VPIN_WIRE_DONE: ok = h.cnt == 0 && h.payload_len == 0; break;
    default: ok = h.cnt == 0 && h.payload_len >= 4 && h.payload_len <= 4 + VPIN_WIRE_MAX_TEXT; break;
  }
  if (!ok) {
    snprintf(why, sizeof why, "%s: payload_len %llu is not what type %u and cnt %u imply", who, (unsigned long long)h.payload_len,
             (unsigned)h.type, (unsigned)h.cnt);
    return fail(VPIN_EINVAL, why);
  }
  return VPIN_OK;
}

}  // namespace

}  // namespace vpin::wire

using namespace vpin::wire;

extern "C" {

int vpin_wire_header_encode(const vpin_wire_header* h, uint8_t out24[VPIN_WIRE_HEADER_LEN]) {
  if (!h || !out24) return fail(VPIN_EINVAL, "vpin_wire_header_encode: null argument");
  const int rc = check(*h, "vpin_wire_header_encode");
  if (rc) return rc;
  memcpy(out24, kMagic, 4);
  out24[4] = h->type; out24[5] = h->flags; out24[6] = h->shift_bits; out24[7] = 0;
  put_le(out24 + 8, h->round, 4);
  put_le(out24 + 12, h->cnt, 4);
  put_le(out24 + 16, h->payload_len, 8);
  return VPIN_OK;
}

int vpin_wire_header_decode(const uint8_t in24[VPIN_WIRE_HEADER_LEN], vpin_wire_header* h) {
  if (!in24 || !h) return fail(VPIN_EINVAL, "vpin_wire_header_decode: null argument");
  if (memcmp(in24, kMagic, 4)) return fail(VPIN_EINVAL, "vpin_wire_header_decode: wrong magic");
  vpin_wire_header t;
  memset(&t, 0, sizeof t);
  t.type = in24[4]; t.flags = in24[5]; t.shift_bits = in24[6];
  t.round = (uint32_t)get_le(in24 + 8, 4);
  t.cnt = (uint32_t)get_le(in24 + 12, 4);
  t.payload_len = get_le(in24 + 16, 8);
  if (t.type < VPIN_WIRE_HELLO || t.type > VPIN_WIRE_ERROR) return check(t, "vpin_wire_header_decode");  // unknown type
  if (in24[7]) return fail(VPIN_EINVAL, "vpin_wire_header_decode: the reserved byte is not zero");
  const int rc = check(t, "vpin_wire_header_decode");
  if (rc) return rc;
  *h = t;
  return VPIN_OK;
}

}  // extern "C"
