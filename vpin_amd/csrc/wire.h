// wire.h -- the byte stream of an encrypted inference between two processes: the frame codec (wire_codec.cpp), the stream and
// its descriptor transport (wire_stream.cpp) and what the two endpoints (wire_net.cpp, infer_client.cpp) take from them.  The
// codec and the stream are plain C++ over include/vpin_hip.h: no HIP, no context, no GPU.  They parse what an untrusted peer
// sends, so tools/wire_check links these two files alone and runs them under the host compiler's sanitizers.
#pragma once
#include <array>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/vpin_hip.h"

struct vpin_wire {
  vpin_wire_io io = {nullptr, nullptr, nullptr};
  int rfd = -1, wfd = -1, timeout_ms = 0;  // the descriptor form: io.user is this object
  bool w_is_socket = false;
  uint64_t stats[4] = {0, 0, 0, 0};  // bytes sent, bytes received, frames sent, frames received
  vpin_ctx* ctx = nullptr;           // the context vpin_wire_round packs and unpacks on (vpin_wire_bind_ctx, vpin_net_serve)
  // host-clock ms per slot (0: HELLO and INPUT, 1 + r: round r): pack, unpack, send, receive of a payload whose header is in
  std::vector<std::array<double, 4>> ms;
};

namespace vpin::wire {

// The text vpin_last_error() gives for a rejection.  The library defines it over its thread's error text (wire_net.cpp); a
// program that links the codec and the stream alone brings its own, and its own vpin_last_error()
void set_error(const char* text);
int fail(int code, const char* text);  // set_error and return code

enum Slot { kPack = 0, kUnpack = 1, kSend = 2, kRecv = 3 };
struct Lap {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double operator()() {
    const auto n = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(n - t).count();
    t = n;
    return ms;
  }
};
void add_ms(vpin_wire* w, size_t slot, Slot what, double ms);

// exactly n bytes through the transport, counted
int send_all(vpin_wire* w, const void* p, size_t n);
int recv_all(vpin_wire* w, void* p, size_t n);
// header (validated by encode) and payload
int send_frame(vpin_wire* w, const vpin_wire_header& h, const void* payload);
// 24 bytes through decode: nothing is allocated from payload_len before decode has accepted the header
int recv_header(vpin_wire* w, vpin_wire_header* h);
int recv_payload(vpin_wire* w, const vpin_wire_header& h, std::vector<uint8_t>* payload);
int discard_payload(vpin_wire* w, const vpin_wire_header& h);  // reads it in pieces into nothing
// an ERROR frame with the code and at most VPIN_WIRE_MAX_TEXT bytes of the text, best effort: the caller's error text stays
void send_error(vpin_wire* w, int code, const char* text);
// the payload of a received ERROR frame as VPIN_ECOMM quoting the peer's code and text
int peer_error(vpin_wire* w, const vpin_wire_header& h, const char* who);


// what the endpoints share (wire_net.cpp; these reach the device through vpin_e2_pack / vpin_e2_unpack): c1 | c2 as one run of
// 2 cnt packed points and back, and a frame's send and payload receive, each timed into the wire's slot
int pack_pair_timed(vpin_wire* w, size_t slot, vpin_ctx* c, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                    const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, std::vector<uint8_t>* out);
int unpack_pair_timed(vpin_wire* w, size_t slot, vpin_ctx* c, const std::vector<uint8_t>& in, size_t cnt, uint8_t* c1x, uint8_t* c1y,
                      uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf);
int send_frame_timed(vpin_wire* w, size_t slot, const vpin_wire_header& h, const void* payload);
int recv_payload_timed(vpin_wire* w, size_t slot, const vpin_wire_header& h, std::vector<uint8_t>* payload);

}  // namespace vpin::wire
