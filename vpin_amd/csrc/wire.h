// wire.h -- the byte stream of an encrypted inference between two processes: the frame codec (wire_codec.cpp), the stream and
// its descriptor transport (wire_stream.cpp) and what the two endpoints (wire_net.cpp, infer_client.cpp) take from them.  The
// codec and the stream are plain C++ over include/vpin_hip.h: no HIP, no context, no GPU.  They parse what an untrusted peer
// sends, so tools/wire_check links these two files alone and runs them under the host compiler's sanitizers.
#pragma once
#include <array>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
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


// ---- the roster of several clients in one batch (wire_roster.cpp: plain C++ like the codec and the stream) -----------------
// Who gets which bytes.  A packed batch is c1 | c2 of all its images: 2 * images * per packed points of 32 bytes, each half
// image-major, `per` the ciphertexts of one image.  A client's frame holds the c1 part of its images and then their c2 part.
struct Peer {
  vpin_wire* w = nullptr;
  size_t wire = 0;           // its index among the caller's wires, and into the status
  size_t first = 0, n = 0;   // its image slots [first, first + n): for its status, its keys and its bias r, for the whole call
  bool live = true;
  // where its images stand in the batch at hand: at `at`, `present` of them.  first and n until images leave the batch
  // (Roster::rebase, the isolated server); slice, place, copy_images and exchange go by these
  size_t at = 0, present = 0;
};
struct Roster {
  const char* who = "";      // the entry point's name, in front of every text
  size_t max_batch = 0, images = 0;  // images: the slots given out
  size_t batch = 0;                  // the images in the batch at hand: `images` until some leave
  std::vector<Peer> peers;   // the admitted clients, in wire order
  vpin_net_peer_status* status = nullptr;  // one per wire of the caller's
  size_t live() const;
  // the next admitted client: its slots are the n_images after those taken (the caller has seen that they fit)
  void admit(vpin_wire* w, size_t wire, size_t n_images);
  // wire's status: code, stage and "<who>: <text>"; the slots stay as they are
  void report(size_t wire, int code, int stage, const std::string& text);
  // peer p leaves at `stage`: report, and ERROR to it best effort, unless it has said ERROR itself (tell = false)
  void drop(size_t p, int code, int stage, const std::string& text, bool tell = true);
  // the batch at hand holds the images `slots` (ascending): every client's position among them and how many of its images are there
  void rebase(const uint32_t* slots, size_t n);
  // (the isolated server, before a round) the live clients that lost an image to a layer (image_status[slot].code != 0, the
  // driver's) leave at VPIN_NET_STAGE_LAYER with the code and the text of their first such image; the images of the clients so dropped
  size_t drop_refused(const vpin_net_image_status* image_status);
  // (after a round) the slots still in the batch whose client is gone, client after client: peer, its slots
  std::vector<std::pair<size_t, std::vector<uint32_t>>> gone(const uint32_t* slots) const;
};
// peer's frame out of a packed batch, and a frame's points into their places in one
void slice(const Roster& r, const Peer& p, const uint8_t* packed, size_t per, std::vector<uint8_t>* frame);
void place(const Roster& r, const Peer& p, const uint8_t* frame, size_t per, uint8_t* packed);
// the images of peer p out of an image-major array of `elem` bytes per ciphertext into the same places of another
void copy_images(const Peer& p, size_t per, size_t elem, const uint8_t* from, uint8_t* to);
// HELLO and INPUT off one wire that may ask for at most `room` images: the packed key, the packed input (c1 part, then c2 part)
// and its images.  *told: the peer has sent ERROR itself
int read_client(vpin_wire* w, size_t per, size_t room, std::vector<uint8_t>* hello, std::vector<uint8_t>* input,
                size_t* n_images, bool* told);
// One round with every live client: ROUND with its slice to each, all sent first; then the REPLYs in wire order into *reply,
// which is laid out as `packed` (left empty when the round encrypts nothing).  A client whose stream fails, who sends ERROR or
// a REPLY for another round or with another cnt is dropped; the places of every client that is not live hold what the server
// sent.  VPIN_ECOMM when no client is left
int exchange(Roster* r, int round, int flags, int shift_bits, const uint8_t* packed, size_t per, std::vector<uint8_t>* reply);
// DONE to every live client: VPIN_OK and VPIN_NET_STAGE_DONE into its status; one that cannot be told is dropped.  The clients told
size_t finish(Roster* r);

// ---- proof records behind DONE (wire_proof.cpp: plain C++ like the codec and the stream) -----------------------------------
// 40 bytes through vpin_proof_header_decode: nothing is allocated from the lengths before decode has accepted the header
int recv_proof_header(vpin_wire* w, vpin_proof_header* h);
int send_proof(vpin_wire* w, const vpin_proof_header& h, const void* payload);
// an ERROR record with the code and at most VPIN_WIRE_MAX_TEXT bytes of the text, best effort: the caller's error text stays
void send_proof_error(vpin_wire* w, int code, const char* text);
struct ProofRecord {
  vpin_proof_header h;
  std::vector<uint8_t> payload;  // proof | comm | comm_para | comm_input
  const uint8_t* proof() const { return payload.data(); }
  const uint8_t* comm() const { return payload.data() + h.proof_len; }
  const uint8_t* comm_para() const { return comm() + h.comm_len; }
  const uint8_t* comm_input() const { return comm_para() + (payload.size() - h.proof_len - h.comm_len) / 2; }
};
// The client's receiving state machine: n_images * n_expect PROOF records, each the next expected (image, label, is_mult, n_ops),
// then END with that count.  A record that is not the next expected one, or an early or miscounted END, is answered with an ERROR
// record and VPIN_ESHAPE naming both sides before its payload is read; a peer's ERROR is VPIN_ECOMM quoting it.  *out holds the
// records received so far, in order.  ms_recv (may be NULL): host-clock ms spent receiving
int recv_proofs(vpin_wire* w, const char* who, size_t n_images, const vpin_proof_expect* expect, size_t n_expect,
                std::vector<ProofRecord>* out, double* ms_recv);

// what the endpoints share (wire_net.cpp; these reach the device through vpin_e2_pack / vpin_e2_unpack): c1 | c2 as one run of
// 2 cnt packed points and back, and a frame's send and payload receive, each timed into the wire's slot
int pack_pair(vpin_ctx* c, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y,
              const uint8_t* c2inf, size_t cnt, std::vector<uint8_t>* out);
// vpin_e2_unpack (e2_wire.hip) with the rule byte of every point in bad[cnt] instead of a failure on the first: 0, or what
// unpack_rule_text says.  A bad point comes out as zeros
int unpack_rules(vpin_ctx* c, const uint8_t* in32, size_t cnt, uint8_t* px, uint8_t* py, uint8_t* pinf, uint8_t* bad);
const char* unpack_rule_text(uint8_t rule);
int pack_pair_timed(vpin_wire* w, size_t slot, vpin_ctx* c, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                    const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, std::vector<uint8_t>* out);
int unpack_pair_timed(vpin_wire* w, size_t slot, vpin_ctx* c, const std::vector<uint8_t>& in, size_t cnt, uint8_t* c1x, uint8_t* c1y,
                      uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf);
int send_frame_timed(vpin_wire* w, size_t slot, const vpin_wire_header& h, const void* payload);
int recv_payload_timed(vpin_wire* w, size_t slot, const vpin_wire_header& h, std::vector<uint8_t>* payload);

}  // namespace vpin::wire
