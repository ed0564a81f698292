// proof_check.cpp -- the proof records behind DONE under the host compiler's sanitizers.  The record codec and the client's
// receiving state machine (vpin_amd/csrc/wire_proof.cpp) parse what an untrusted server sends.  This program links that file with
// wire_codec.cpp and wire_stream.cpp alone: no HIP, no Python, no GPU, and the verification taken out -- what is checked is which
// records the client takes off the stream and what it answers.  It is run by hand on a CPU machine and is part of no test suite.
// From the repository's root:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//       tools/wire_check/proof_check.cpp vpin_amd/csrc/wire_proof.cpp vpin_amd/csrc/wire_codec.cpp vpin_amd/csrc/wire_stream.cpp \
//       -o tools/wire_check/proof_check && tools/wire_check/proof_check
//
// (the clang++ of ROCm's LLVM serves).  The server is a script over vpin_wire_io callbacks in memory: everything it will ever send
// waits in a buffer, everything the client sends is kept.  It does three things and prints one line for each:
//   1. 200000 seeded headers, from random bytes to good headers with one field spoiled: decode either names a rule, or accepts a
//      header that encode gives back byte for byte and whose payload is within the bound of its shape;
//   2. an honest stream of 2 images x 3 records and END cut at every offset: the full stream is VPIN_OK with all six records, every
//      cut is VPIN_ECOMM, nothing is read past the cut and nothing is answered;
//   3. scripted servers: a wrong order, a wrong n_ops, another image, END early, END with a wrong count, a record too many, ERROR
//      in the middle and a header that breaks a rule: the code, the text naming both sides, the ERROR record the client answers
//      with, and not one byte read past the header that was refused.
// Exit status 0 and "proof_check: ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vpin_amd/csrc/wire.h"

// what the library defines over its own error text
static thread_local std::string g_error;
namespace vpin::wire {
void set_error(const char* text) { g_error = text; }
}  // namespace vpin::wire
extern "C" const char* vpin_last_error(void) { return g_error.c_str(); }

#define CHECK(cond)                                                                                    \
  do {                                                                                                 \
    if (!(cond)) {                                                                                     \
      fprintf(stderr, "proof_check: %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, vpin_last_error()); \
      exit(1);                                                                                         \
    }                                                                                                  \
  } while (0)

using namespace vpin::wire;

namespace {

uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// a server in memory
struct Script {
  std::vector<uint8_t> in, out;  // what the client will read, what it wrote
  size_t pos = 0;
};
int mem_send(void* user, const void* p, size_t n) {
  Script* s = (Script*)user;
  s->out.insert(s->out.end(), (const uint8_t*)p, (const uint8_t*)p + n);
  return 0;
}
int mem_recv(void* user, void* p, size_t n) {
  Script* s = (Script*)user;
  if (s->in.size() - s->pos < n) {
    s->pos = s->in.size();
    return fail(VPIN_ECOMM, "script: the stream ended");
  }
  memcpy(p, s->in.data() + s->pos, n);
  s->pos += n;
  return 0;
}

vpin_proof_header record_header(int is_mult, uint64_t n_ops, uint32_t image, uint32_t label, uint64_t proof_len) {
  vpin_proof_header h;
  memset(&h, 0, sizeof h);
  h.kind = VPIN_PROOF_RECORD; h.is_mult = (uint8_t)is_mult; h.image = image; h.label = label; h.n_ops = n_ops;
  h.proof_len = proof_len; h.comm_len = vpin_gadget_comm_bytes(is_mult, (size_t)n_ops);
  return h;
}

void append_header(std::vector<uint8_t>* to, const vpin_proof_header& h) {
  uint8_t head[VPIN_PROOF_HEADER_LEN];
  CHECK(vpin_proof_header_encode(&h, head) == VPIN_OK);
  to->insert(to->end(), head, head + sizeof head);
}

void append_record(std::vector<uint8_t>* to, const vpin_proof_header& h, uint64_t seed) {
  append_header(to, h);
  for (uint64_t i = 0, n = vpin_proof_payload_len(&h); i < n; i++) to->push_back((uint8_t)splitmix(&seed));
}

void append_end(std::vector<uint8_t>* to, uint32_t count) {
  vpin_proof_header h;
  memset(&h, 0, sizeof h);
  h.kind = VPIN_PROOF_END; h.image = count;
  append_header(to, h);
}

void append_error(std::vector<uint8_t>* to, int code, const char* text) {
  vpin_proof_header h;
  memset(&h, 0, sizeof h);
  h.kind = VPIN_PROOF_ERROR; h.proof_len = 4 + strlen(text);
  append_header(to, h);
  const uint32_t c = (uint32_t)(int32_t)code;
  for (int i = 0; i < 4; i++) to->push_back((uint8_t)(c >> (8 * i)));
  to->insert(to->end(), text, text + strlen(text));
}

// the client's list: per image one label of 3 multiplications and 5 additions, and a per-layer label of 2 additions
const vpin_proof_expect kExpect[3] = {{0, 1, 3}, {0, 0, 5}, {1, 0, 2}};
constexpr size_t kImages = 2, kExpectN = 3;

vpin_proof_header expected(size_t at, uint64_t proof_len) {
  const vpin_proof_expect& e = kExpect[at % kExpectN];
  return record_header(e.is_mult, e.n_ops, (uint32_t)(at / kExpectN), e.label, proof_len);
}

struct Run {
  int rc;
  std::string text;
  std::vector<ProofRecord> recs;
  size_t read, frames;
  std::vector<uint8_t> answered;
};
Run run(const std::vector<uint8_t>& stream) {
  Script s;
  s.in = stream;
  const vpin_wire_io io = {mem_send, mem_recv, &s};
  vpin_wire* w = nullptr;
  CHECK(vpin_wire_create(&io, &w) == VPIN_OK);
  Run r;
  g_error.clear();
  r.rc = recv_proofs(w, "proof_check", kImages, kExpect, kExpectN, &r.recs, nullptr);
  r.text = vpin_last_error();
  uint64_t st[4];
  CHECK(vpin_wire_stats(w, st) == VPIN_OK);
  CHECK(st[1] == s.pos || r.rc == VPIN_ECOMM);  // every byte taken off the script is counted
  r.read = s.pos; r.frames = (size_t)st[3]; r.answered = s.out;
  vpin_wire_free(w);
  return r;
}

// what the client answered: nothing, or one ERROR record with this code whose text holds `text`
bool answered_error(const Run& r, int code, const char* text) {
  if (r.answered.size() < VPIN_PROOF_HEADER_LEN) return false;
  vpin_proof_header h;
  if (vpin_proof_header_decode(r.answered.data(), &h) != VPIN_OK || h.kind != VPIN_PROOF_ERROR) return false;
  if (r.answered.size() != VPIN_PROOF_HEADER_LEN + h.proof_len) return false;
  uint32_t c = 0;
  for (int i = 0; i < 4; i++) c |= (uint32_t)r.answered[VPIN_PROOF_HEADER_LEN + i] << (8 * i);
  const std::string said((const char*)r.answered.data() + VPIN_PROOF_HEADER_LEN + 4, (size_t)h.proof_len - 4);
  return (int)(int32_t)c == code && said.find(text) != std::string::npos;
}

// ---- 1. hostile headers ------------------------------------------------------------------------------------------------------------
void hostile_headers() {
  uint64_t seed = 0x5eed0001, accepted = 0, rejected = 0;
  // no payload may exceed that of the largest shape
  uint64_t bound = 0;
  for (int m = 0; m < 2; m++) {
    const uint64_t b = vpin_gadget_proof_max_bytes(m, VPIN_PROOF_MAX_OPS) + vpin_gadget_comm_bytes(m, VPIN_PROOF_MAX_OPS) +
                       64 * (uint64_t)vpin_gadget_vars_rows(m, VPIN_PROOF_MAX_OPS);
    bound = b > bound ? b : bound;
  }
  for (int it = 0; it < 200000; it++) {
    uint8_t b[VPIN_PROOF_HEADER_LEN];
    for (size_t i = 0; i < sizeof b; i += 8) {
      const uint64_t v = splitmix(&seed);
      memcpy(b + i, &v, 8);
    }
    const uint64_t how = splitmix(&seed);
    if (how % 8) memcpy(b, "VPP1", 4);  // most get past the magic
    if (how % 8 > 1) {                   // and many are a good header with one field spoiled, or none
      const int m = (int)(splitmix(&seed) & 1);
      const uint64_t n = 1 + splitmix(&seed) % (how % 16 > 8 ? VPIN_PROOF_MAX_OPS : 4096);
      vpin_proof_header h = record_header(m, n, (uint32_t)splitmix(&seed), (uint32_t)splitmix(&seed), splitmix(&seed) % (vpin_gadget_proof_max_bytes(m, (size_t)n) + 1));
      if (how % 5 == 1) { memset(&h, 0, sizeof h); h.kind = VPIN_PROOF_END; h.image = (uint32_t)splitmix(&seed); }
      if (how % 5 == 2) { memset(&h, 0, sizeof h); h.kind = VPIN_PROOF_ERROR; h.proof_len = 4 + splitmix(&seed) % (VPIN_WIRE_MAX_TEXT + 1); }
      CHECK(vpin_proof_header_encode(&h, b) == VPIN_OK);
      const uint64_t spoil = splitmix(&seed) % 48;
      if (spoil < VPIN_PROOF_HEADER_LEN) b[spoil] ^= (uint8_t)(1u << (splitmix(&seed) % 8));
    }
    vpin_proof_header h;
    g_error.clear();
    const int rc = vpin_proof_header_decode(b, &h);
    if (rc) {
      CHECK(rc == VPIN_EINVAL && g_error.find("vpin_proof_header_decode: ") == 0 && g_error.size() > 26);
      rejected++;
      continue;
    }
    uint8_t again[VPIN_PROOF_HEADER_LEN];
    CHECK(vpin_proof_header_encode(&h, again) == VPIN_OK && !memcmp(again, b, sizeof b));
    CHECK(vpin_proof_payload_len(&h) <= bound);
    accepted++;
  }
  CHECK(accepted > 10000 && rejected > 10000);
  printf("proof_check: 200000 seeded headers: %llu accepted and encoded back byte for byte, %llu rejected by a named rule; no payload above %llu bytes\n",
         (unsigned long long)accepted, (unsigned long long)rejected, (unsigned long long)bound);
}

// ---- 2. an honest stream cut at every offset ---------------------------------------------------------------------------------------
std::vector<uint8_t> honest_stream() {
  std::vector<uint8_t> s;
  for (size_t at = 0; at < kImages * kExpectN; at++) append_record(&s, expected(at, 90 + 7 * at), 0xabc0 + at);
  append_end(&s, (uint32_t)(kImages * kExpectN));
  return s;
}

void cut_everywhere() {
  const std::vector<uint8_t> all = honest_stream();
  const Run whole = run(all);
  CHECK(whole.rc == VPIN_OK && whole.recs.size() == kImages * kExpectN && whole.read == all.size() && whole.answered.empty());
  CHECK(whole.frames == kImages * kExpectN + 1);
  size_t at = 0;
  for (size_t k = 0; k < whole.recs.size(); k++) {  // the records hold the stream's bytes
    const ProofRecord& r = whole.recs[k];
    CHECK(r.h.image == k / kExpectN && r.h.n_ops == kExpect[k % kExpectN].n_ops && r.h.proof_len == 90 + 7 * k);
    CHECK(r.payload.size() == vpin_proof_payload_len(&r.h) && !memcmp(r.payload.data(), all.data() + at + VPIN_PROOF_HEADER_LEN, r.payload.size()));
    CHECK(r.comm() == r.payload.data() + r.h.proof_len && r.comm_input() + 32 * vpin_gadget_vars_rows(r.h.is_mult, (size_t)r.h.n_ops) == r.payload.data() + r.payload.size());
    at += VPIN_PROOF_HEADER_LEN + r.payload.size();
  }
  for (size_t cut = 0; cut < all.size(); cut++) {
    const Run r = run(std::vector<uint8_t>(all.begin(), all.begin() + cut));
    CHECK(r.rc == VPIN_ECOMM && r.text.find("proof_check: ") == 0 && r.answered.empty() && r.recs.size() <= kImages * kExpectN);
  }
  printf("proof_check: an honest stream of %zu records and END (%zu bytes): VPIN_OK whole, VPIN_ECOMM at each of %zu cuts\n", whole.recs.size(),
         all.size(), all.size());
}

// ---- 3. scripted servers -----------------------------------------------------------------------------------------------------------
void scripted_servers() {
  size_t cases = 0;
  // the stream up to record `good`, then `bad`: refused with VPIN_ESHAPE at bad's header, which is the last thing read
  auto refused = [&](size_t good, const std::vector<uint8_t>& bad, const char* text) {
    std::vector<uint8_t> s;
    for (size_t at = 0; at < good; at++) append_record(&s, expected(at, 50), 0xdef0 + at);
    const size_t upto = s.size() + VPIN_PROOF_HEADER_LEN;
    s.insert(s.end(), bad.begin(), bad.end());
    const Run r = run(s);
    CHECK(r.rc == VPIN_ESHAPE && r.text.find(text) != std::string::npos && r.text.find("proof_check: ") == 0);
    CHECK(r.read == upto && r.recs.size() == good);  // nothing of the refused record's payload, and nothing was allocated for it
    CHECK(answered_error(r, VPIN_ESHAPE, text));
    cases++;
  };
  auto rec = [](const vpin_proof_header& h) {
    std::vector<uint8_t> b;
    append_record(&b, h, 0x777);
    return b;
  };
  for (size_t good = 0; good < kImages * kExpectN; good++) {
    const vpin_proof_expect& e = kExpect[good % kExpectN];
    const uint32_t image = (uint32_t)(good / kExpectN);
    char text[200];
    // a wrong order: the record that should come one later (at the end of an image: the next image's first)
    const vpin_proof_header next = expected((good + 1) % (kImages * kExpectN), 50);
    if (next.image != image || next.label != e.label)
      snprintf(text, sizeof text, "the server sends image %u, label %u, the expectation says image %u, label %u comes next", next.image, next.label, image, e.label);
    else
      snprintf(text, sizeof text, "image %u, label %u: the server proves %llu %s, the expectation says %llu", image, e.label, (unsigned long long)next.n_ops,
               next.is_mult ? "multiplications" : "additions", (unsigned long long)e.n_ops);
    refused(good, rec(next), text);
    // a wrong n_ops
    snprintf(text, sizeof text, "image %u, label %u: the server proves %llu %s, the expectation says %llu", image, e.label, (unsigned long long)e.n_ops + 1,
             e.is_mult ? "multiplications" : "additions", (unsigned long long)e.n_ops);
    refused(good, rec(record_header(e.is_mult, e.n_ops + 1, image, e.label, 50)), text);
    // the other kind of operation
    snprintf(text, sizeof text, "the expectation says %llu %s", (unsigned long long)e.n_ops, e.is_mult ? "multiplications" : "additions");
    refused(good, rec(record_header(!e.is_mult, e.n_ops, image, e.label, 50)), text);
    // another image
    snprintf(text, sizeof text, "the server sends image %u, label %u, the expectation says image %u", image + 1, e.label, image);
    refused(good, rec(record_header(e.is_mult, e.n_ops, image + 1, e.label, 50)), text);
    // END early
    std::vector<uint8_t> end;
    append_end(&end, (uint32_t)good);
    snprintf(text, sizeof text, "the server ends after %zu of %zu proofs", good, kImages * kExpectN);
    refused(good, end, text);
  }
  for (uint32_t count : {0u, 5u, 7u, 0xffffffffu}) {  // END with a wrong count
    std::vector<uint8_t> end;
    append_end(&end, count);
    char text[120];
    snprintf(text, sizeof text, "the server's END counts %u proofs, %zu were sent", count, kImages * kExpectN);
    refused(kImages * kExpectN, end, text);
  }
  refused(kImages * kExpectN, rec(expected(0, 50)), "the server sends a proof behind the 6 the expectation lists");
  // ERROR in the middle, and at the start: VPIN_ECOMM quoting it, nothing answered
  for (size_t good : {(size_t)0, (size_t)2, kImages * kExpectN}) {
    std::vector<uint8_t> s;
    for (size_t at = 0; at < good; at++) append_record(&s, expected(at, 50), 0xdef0 + at);
    append_error(&s, VPIN_EVERIFY, "the witness does not satisfy the gadget");
    const Run r = run(s);
    CHECK(r.rc == VPIN_ECOMM && r.text == "proof_check: the peer reported an error (-6): the witness does not satisfy the gadget");
    CHECK(r.read == s.size() && r.answered.empty() && r.recs.size() == good);
    cases++;
  }
  // a header that breaks a rule of the codec: VPIN_EINVAL naming it, answered, and nothing more read
  {
    std::vector<uint8_t> s;
    append_record(&s, expected(0, 50), 0xdef0);
    vpin_proof_header h = expected(1, 50);
    std::vector<uint8_t> bad;
    append_header(&bad, h);
    const uint64_t huge = (uint64_t)1 << 62;
    for (int i = 0; i < 8; i++) bad[24 + i] = (uint8_t)(huge >> (8 * i));  // proof_len
    const size_t upto = s.size() + VPIN_PROOF_HEADER_LEN;
    s.insert(s.end(), bad.begin(), bad.end());
    s.resize(s.size() + 4096, 0x5a);
    const Run r = run(s);
    CHECK(r.rc == VPIN_EINVAL && r.text.find("proof_check: vpin_proof_header_decode: proof_len 4611686018427387904 is above") == 0);
    CHECK(r.read == upto && r.recs.size() == 1 && answered_error(r, VPIN_EINVAL, "proof_len 4611686018427387904 is above"));
    cases++;
  }
  printf("proof_check: %zu scripted servers (wrong order, wrong n_ops, other kind, other image, END early, END miscounted, a record too many, "
         "ERROR, a broken header): each refused with its code and text at the header, and answered as specified\n", cases);
}

}  // namespace

int main() {
  hostile_headers();
  cut_everywhere();
  scripted_servers();
  printf("proof_check: ok\n");
  return 0;
}
