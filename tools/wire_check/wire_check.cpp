// wire_check.cpp -- the frame codec and the descriptor stream of the inference wire under the host compiler's sanitizers.
// Both parse bytes from an untrusted peer.  This program links vpin_amd/csrc/wire_codec.cpp and wire_stream.cpp alone: no HIP,
// no Python, no GPU.  It is run by hand on a CPU machine and is part of no test suite.  From the repository's root:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -I include \
//       tools/wire_check/wire_check.cpp vpin_amd/csrc/wire_codec.cpp vpin_amd/csrc/wire_stream.cpp -o tools/wire_check/wire_check \
//       && tools/wire_check/wire_check
//
// (the clang++ of ROCm's LLVM serves).  It does three things and prints one line for each:
//   1. every truncation of one valid frame of each type: a stream that ends after k bytes is VPIN_ECOMM naming k, never a
//      read past the end, and the whole frame is accepted;
//   2. 10^5 seeded random mutations of valid headers: decode either rejects with a text or accepts a header that encodes back
//      to the same 24 bytes;
//   3. a frame exchange over a socketpair between two threads, the peer closing at every byte offset of a short frame: the
//      receiver returns VPIN_ECOMM with the offset, the sender to a closed peer returns VPIN_ECOMM, and no SIGPIPE ends the process.
// Exit status 0 and "wire_check: ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <sys/socket.h>
#include <unistd.h>

#include "../../vpin_amd/csrc/wire.h"

// what the library defines over its own error text
static thread_local std::string g_error;
namespace vpin::wire {
void set_error(const char* text) { g_error = text; }
}  // namespace vpin::wire
extern "C" const char* vpin_last_error(void) { return g_error.c_str(); }

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      fprintf(stderr, "wire_check: %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, vpin_last_error()); \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

namespace {

struct Frame {
  vpin_wire_header h;
  std::vector<uint8_t> bytes;  // header and payload
};

Frame make(uint8_t type, uint32_t cnt, uint64_t payload_len) {
  Frame f;
  memset(&f.h, 0, sizeof f.h);
  f.h.type = type; f.h.flags = 3; f.h.shift_bits = 26; f.h.round = 4; f.h.cnt = cnt; f.h.payload_len = payload_len;
  f.bytes.resize(VPIN_WIRE_HEADER_LEN + payload_len);
  CHECK(vpin_wire_header_encode(&f.h, f.bytes.data()) == VPIN_OK);
  for (size_t i = VPIN_WIRE_HEADER_LEN; i < f.bytes.size(); i++) f.bytes[i] = (uint8_t)(7 * i + 1);
  return f;
}

std::vector<Frame> one_of_each() {
  return {make(VPIN_WIRE_HELLO, 1, 32), make(VPIN_WIRE_INPUT, 3, 192), make(VPIN_WIRE_ROUND, 2, 128), make(VPIN_WIRE_REPLY, 2, 128),
          make(VPIN_WIRE_REPLY, 0, 0),  make(VPIN_WIRE_DONE, 0, 0),    make(VPIN_WIRE_ERROR, 0, 4 + 11)};
}

// a transport over a buffer of exactly the bytes a truncated stream delivers
struct Mem {
  const uint8_t* p;
  size_t n, pos;
};
int mem_recv(void* user, void* out, size_t n) {
  Mem* m = (Mem*)user;
  if (m->n - m->pos < n) {
    char why[96];
    snprintf(why, sizeof why, "the stream ended after %zu of %zu bytes", m->n - m->pos, n);
    vpin::wire::set_error(why);
    m->pos = m->n;
    return VPIN_ECOMM;
  }
  memcpy(out, m->p + m->pos, n);
  m->pos += n;
  return 0;
}
int mem_send(void*, const void*, size_t) { return VPIN_ECOMM; }

void truncations() {
  size_t cases = 0;
  for (const Frame& f : one_of_each()) {
    for (size_t k = 0; k <= f.bytes.size(); k++, cases++) {
      // the receiver's buffer is exactly as long as the payload: a byte too many is the sanitizer's to see
      std::vector<uint8_t> exact(f.bytes.begin(), f.bytes.begin() + k), payload((size_t)f.h.payload_len);
      Mem m{exact.data(), exact.size(), 0};
      vpin_wire_io io{mem_send, mem_recv, &m};
      vpin_wire* w = nullptr;
      CHECK(vpin_wire_create(&io, &w) == VPIN_OK);
      vpin_wire_header h;
      const int rc = vpin_wire_recv(w, &h, payload.data(), payload.size());
      if (k < f.bytes.size()) {
        CHECK(rc == VPIN_ECOMM && strstr(vpin_last_error(), "the stream ended after"));
      } else {
        CHECK(rc == VPIN_OK && h.type == f.h.type && h.cnt == f.h.cnt && h.payload_len == f.h.payload_len);
        CHECK(payload.empty() || !memcmp(payload.data(), f.bytes.data() + VPIN_WIRE_HEADER_LEN, payload.size()));
      }
      vpin_wire_free(w);
      // and the header alone through decode, from a buffer of its own
      if (k >= VPIN_WIRE_HEADER_LEN) {
        std::vector<uint8_t> head(f.bytes.begin(), f.bytes.begin() + VPIN_WIRE_HEADER_LEN);
        CHECK(vpin_wire_header_decode(head.data(), &h) == VPIN_OK);
      }
    }
  }
  printf("wire_check: %zu truncations of %zu frames\n", cases, one_of_each().size());
}

uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

void mutations() {
  const std::vector<Frame> frames = one_of_each();
  uint64_t seed = 0x77697265;  // "wire"
  size_t accepted = 0, rejected = 0;
  for (int it = 0; it < 100000; it++) {
    const Frame& f = frames[splitmix(&seed) % frames.size()];
    std::vector<uint8_t> head(f.bytes.begin(), f.bytes.begin() + VPIN_WIRE_HEADER_LEN);  // a heap buffer of exactly 24 bytes
    const int n_mut = 1 + (int)(splitmix(&seed) % 4);
    for (int m = 0; m < n_mut; m++) {
      const uint64_t r = splitmix(&seed);
      const size_t at = (size_t)(r % VPIN_WIRE_HEADER_LEN);
      switch ((r >> 8) % 4) {
        case 0: head[at] ^= (uint8_t)(1u << ((r >> 16) % 8)); break;
        case 1: head[at] = (uint8_t)(r >> 16); break;
        case 2: head[at] = 0xff; break;
        default: head[at] = 0; break;
      }
    }
    vpin_wire_header h;
    g_error.clear();
    const int rc = vpin_wire_header_decode(head.data(), &h);
    if (rc == VPIN_OK) {
      uint8_t back[VPIN_WIRE_HEADER_LEN];
      CHECK(vpin_wire_header_encode(&h, back) == VPIN_OK && !memcmp(back, head.data(), sizeof back));
      CHECK(h.cnt <= VPIN_WIRE_MAX_CNT && h.payload_len <= 64ull * VPIN_WIRE_MAX_CNT);
      accepted++;
    } else {
      CHECK(rc == VPIN_EINVAL && strstr(vpin_last_error(), "vpin_wire_header_decode: "));
      rejected++;
    }
  }
  printf("wire_check: 100000 mutated headers, %zu accepted, %zu rejected\n", accepted, rejected);
}

void exchange() {
  const Frame f = make(VPIN_WIRE_ROUND, 1, 64);  // 88 bytes
  // whole frames both ways between two threads
  {
    int sv[2];
    CHECK(socketpair(AF_UNIX, SOCK_STREAM, 0, sv) == 0);
    std::thread peer([&] {
      vpin_wire* w = nullptr;
      CHECK(vpin_wire_fd_create(sv[1], sv[1], 2000, &w) == VPIN_OK);
      vpin_wire_header h;
      std::vector<uint8_t> p(64);
      CHECK(vpin_wire_recv(w, &h, p.data(), p.size()) == VPIN_OK && h.type == VPIN_WIRE_ROUND);
      h.type = VPIN_WIRE_REPLY;
      CHECK(vpin_wire_send(w, &h, p.data()) == VPIN_OK);
      CHECK(vpin_wire_send_error(w, VPIN_ESHAPE, "a text") == VPIN_OK);
      vpin_wire_free(w);
    });
    vpin_wire* w = nullptr;
    CHECK(vpin_wire_fd_create(sv[0], sv[0], 2000, &w) == VPIN_OK);
    CHECK(vpin_wire_send(w, &f.h, f.bytes.data() + VPIN_WIRE_HEADER_LEN) == VPIN_OK);
    vpin_wire_header h;
    std::vector<uint8_t> p(64), e(4 + VPIN_WIRE_MAX_TEXT);
    CHECK(vpin_wire_recv(w, &h, p.data(), p.size()) == VPIN_OK && h.type == VPIN_WIRE_REPLY);
    CHECK(!memcmp(p.data(), f.bytes.data() + VPIN_WIRE_HEADER_LEN, 64));
    CHECK(vpin_wire_recv(w, &h, e.data(), e.size()) == VPIN_OK && h.type == VPIN_WIRE_ERROR && h.payload_len == 4 + 6);
    uint64_t st[4];
    CHECK(vpin_wire_stats(w, st) == VPIN_OK && st[0] == 88 && st[1] == 88 + 24 + 10 && st[2] == 1 && st[3] == 2);
    peer.join();
    vpin_wire_free(w);
    close(sv[0]); close(sv[1]);
  }
  // the peer writes k bytes of the frame and closes, for every k short of the whole
  for (size_t k = 0; k < f.bytes.size(); k++) {
    int sv[2];
    CHECK(socketpair(AF_UNIX, SOCK_STREAM, 0, sv) == 0);
    std::thread peer([&] {
      CHECK(k == 0 || write(sv[1], f.bytes.data(), k) == (ssize_t)k);
      close(sv[1]);
    });
    vpin_wire* w = nullptr;
    CHECK(vpin_wire_fd_create(sv[0], sv[0], 2000, &w) == VPIN_OK);
    vpin_wire_header h;
    std::vector<uint8_t> p(64);
    CHECK(vpin_wire_recv(w, &h, p.data(), p.size()) == VPIN_ECOMM);
    char want[64];
    if (k < VPIN_WIRE_HEADER_LEN) snprintf(want, sizeof want, "closed the stream after %zu of 24 bytes", k);
    else snprintf(want, sizeof want, "closed the stream after %zu of 64 bytes", k - VPIN_WIRE_HEADER_LEN);
    CHECK(strstr(vpin_last_error(), want));
    peer.join();
    // and a frame sent to the closed peer is an error return: SIGPIPE would have ended the process here
    CHECK(vpin_wire_send(w, &f.h, f.bytes.data() + VPIN_WIRE_HEADER_LEN) == VPIN_ECOMM);
    vpin_wire_free(w);
    close(sv[0]);
  }
  // the same over a pipe, where MSG_NOSIGNAL does not exist: the signal is masked around the write
  {
    int to_peer[2], from_peer[2];
    CHECK(pipe(to_peer) == 0 && pipe(from_peer) == 0);
    close(to_peer[0]);
    close(from_peer[1]);
    vpin_wire* w = nullptr;
    CHECK(vpin_wire_fd_create(from_peer[0], to_peer[1], 500, &w) == VPIN_OK);
    CHECK(vpin_wire_send(w, &f.h, f.bytes.data() + VPIN_WIRE_HEADER_LEN) == VPIN_ECOMM);
    vpin_wire_header h;
    CHECK(vpin_wire_recv(w, &h, nullptr, 0) == VPIN_ECOMM && strstr(vpin_last_error(), "closed the stream after 0 of 24 bytes"));
    vpin_wire_free(w);
    close(to_peer[1]); close(from_peer[0]);
  }
  printf("wire_check: %zu closing offsets of a %zu-byte frame over a socketpair, and a closed pipe\n", f.bytes.size(), f.bytes.size());
}

}  // namespace

int main() {
  truncations();
  mutations();
  exchange();
  printf("wire_check: ok\n");
  return 0;
}
