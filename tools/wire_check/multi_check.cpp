// multi_check.cpp -- the roster of several clients in one batched inference under the host compiler's sanitizers.  The roster
// (vpin_amd/csrc/wire_roster.cpp) decides which client gets which bytes of a round and where a reply's points land, and it
// parses what untrusted peers send.  This program links it with wire_codec.cpp and wire_stream.cpp alone: no HIP, no Python,
// no GPU.  It is run by hand on a CPU machine and is part of no test suite.  From the repository's root:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//       tools/wire_check/multi_check.cpp vpin_amd/csrc/wire_roster.cpp vpin_amd/csrc/wire_codec.cpp vpin_amd/csrc/wire_stream.cpp \
//       -o tools/wire_check/multi_check && tools/wire_check/multi_check
//
// (the clang++ of ROCm's LLVM serves).  The clients are scripts over vpin_wire_io callbacks in memory: everything a client will
// ever send waits in a buffer, everything the server sends it is kept.  The server is the endpoint's loop (wire_multi.cpp) with
// the device taken out: admission by read_client, three rounds by exchange, finish; a "layer" makes an image's next ciphertexts
// from that image's last ones alone, as the real layers do, so what a client is sent depends on nobody else.  It does three things
// and prints one line for each:
//   1. K = 1 .. 5 clients with B_i in 1 .. 3 images (every composition for K <= 3, seeded samples above): every slot, every
//      status, every frame each client receives is that of the same client served alone;
//   2. every client of such a roster dropped at every stage in turn (a wrong first frame, a stream that ends after HELLO, an INPUT
//      that is no whole image, a stream that ends after INPUT, and in every round an ERROR, a REPLY for another round, a REPLY
//      with another cnt and a frame cut in half): its status names the stage and the code, its images go on as what the server
//      sent, and every other client's bytes are still those of that client alone;
//   3. 2000 seeded rosters with random drops of any number of clients, the same checks; all gone is VPIN_ECOMM.
// Exit status 0 and "multi_check: ok" when all hold.
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
      fprintf(stderr, "multi_check: %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, vpin_last_error()); \
      exit(1);                                                                                         \
    }                                                                                                  \
  } while (0)

using namespace vpin::wire;

namespace {

constexpr size_t kPer = 3, kRounds = 3, kMaxBatch = 15;
constexpr size_t kRoundN[kRounds] = {2, 3, 1};  // ciphertexts per image
constexpr int kRoundFlags[kRounds] = {VPIN_LENET_RELU | VPIN_LENET_REENCRYPT, VPIN_LENET_REENCRYPT, 0};

// the stages a client can fail at
enum Fail { kNone = 0, kFirstFrame, kEndAfterHello, kInputCnt, kEndAfterInput, kRound0 };  // kRound0 + 4 r + {ERROR, round, cnt, cut}
constexpr int kFails = kRound0 + 4 * (int)kRounds;

uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

void fill(std::vector<uint8_t>* out, size_t n, uint64_t seed) {
  out->resize(n);
  for (size_t i = 0; i < n; i++) (*out)[i] = (uint8_t)splitmix(&seed);
}

void append_frame(std::vector<uint8_t>* to, uint8_t type, uint32_t round, uint32_t cnt, const std::vector<uint8_t>& payload, bool cut = false) {
  vpin_wire_header h;
  memset(&h, 0, sizeof h);
  h.type = type; h.round = round; h.cnt = cnt; h.payload_len = payload.size();
  uint8_t head[VPIN_WIRE_HEADER_LEN];
  CHECK(vpin_wire_header_encode(&h, head) == VPIN_OK);
  std::vector<uint8_t> f(head, head + sizeof head);
  f.insert(f.end(), payload.begin(), payload.end());
  to->insert(to->end(), f.begin(), f.begin() + (cut ? f.size() / 2 : f.size()));
}

// one client: who it is, its images, where it fails; all it will ever send, all it is sent
struct Client {
  uint64_t id = 0;
  size_t images = 1;
  int fail = kNone;
  std::vector<uint8_t> in, out;
  size_t pos = 0;
};

void script(Client* c) {
  std::vector<uint8_t> p;
  c->in.clear(); c->out.clear(); c->pos = 0;
  fill(&p, 32, c->id * 1000 + 1);
  if (c->fail == kFirstFrame) { append_frame(&c->in, VPIN_WIRE_DONE, 0, 0, {}); return; }
  append_frame(&c->in, VPIN_WIRE_HELLO, 0, 1, p);
  if (c->fail == kEndAfterHello) return;
  const size_t n_in = c->images * kPer + (c->fail == kInputCnt ? 1 : 0);
  fill(&p, 64 * n_in, c->id * 1000 + 2);
  append_frame(&c->in, VPIN_WIRE_INPUT, 0, (uint32_t)n_in, p);
  if (c->fail == kInputCnt || c->fail == kEndAfterInput) return;
  for (size_t r = 0; r < kRounds; r++) {
    const int how = c->fail - kRound0 - 4 * (int)r;  // 0 .. 3: this round is where it fails
    const size_t cnt = (kRoundFlags[r] & VPIN_LENET_REENCRYPT) ? c->images * kRoundN[r] : 0;
    fill(&p, 64 * cnt, c->id * 1000 + 10 + r);
    if (how == 0) {
      append_frame(&c->in, VPIN_WIRE_ERROR, 0, 0, std::vector<uint8_t>{0xfb, 0xff, 0xff, 0xff, 'n', 'o'});
    } else if (how == 1) {
      append_frame(&c->in, VPIN_WIRE_REPLY, (uint32_t)r + 1, (uint32_t)cnt, p);
    } else if (how == 2) {
      fill(&p, 64 * (cnt + 1), 7);
      append_frame(&c->in, VPIN_WIRE_REPLY, (uint32_t)r, (uint32_t)cnt + 1, p);
    } else {
      append_frame(&c->in, VPIN_WIRE_REPLY, (uint32_t)r, (uint32_t)cnt, p, how == 3);
    }
    if (how >= 0 && how <= 3) return;
  }
}

int mem_recv(void* user, void* out, size_t n) {
  Client* c = (Client*)user;
  if (c->in.size() - c->pos < n) {
    char why[96];
    snprintf(why, sizeof why, "the stream ended after %zu of %zu bytes", c->in.size() - c->pos, n);
    set_error(why);
    c->pos = c->in.size();
    return VPIN_ECOMM;
  }
  memcpy(out, c->in.data() + c->pos, n);
  c->pos += n;
  return 0;
}
int mem_send(void* user, const void* p, size_t n) {
  Client* c = (Client*)user;
  c->out.insert(c->out.end(), (const uint8_t*)p, (const uint8_t*)p + n);
  return 0;
}

// what fail stage f leaves in the client's status
void expected(int f, int* code, int* stage, bool* admitted) {
  *admitted = f == kNone || f >= kEndAfterInput;
  if (f == kNone) { *code = VPIN_OK; *stage = VPIN_NET_STAGE_DONE; return; }
  if (f < kEndAfterInput) { *code = f == kEndAfterHello ? VPIN_ECOMM : VPIN_ESHAPE; *stage = VPIN_NET_STAGE_ADMISSION; return; }
  if (f == kEndAfterInput) { *code = VPIN_ECOMM; *stage = 0; return; }
  const int how = (f - kRound0) % 4;
  *stage = (f - kRound0) / 4;
  *code = how == 1 || how == 2 ? VPIN_ESHAPE : VPIN_ECOMM;
}

// an image's next ciphertexts from its last ones alone: n points per half
void layer(const std::vector<uint8_t>& last, size_t round, size_t n, std::vector<uint8_t>* c1, std::vector<uint8_t>* c2) {
  uint64_t h = 0xcbf29ce484222325ull + round;
  for (uint8_t b : last) h = (h ^ b) * 0x100000001b3ull;
  fill(c1, 32 * n, h);
  fill(c2, 32 * n, h ^ 0x5555);
}

struct Served {
  int rc = VPIN_OK;
  std::vector<vpin_net_peer_status> status;
  size_t images = 0, echoes = 0;  // echoes: rounds in which a dropped client's images were seen to hold what the server sent
};

// the endpoint's loop without the device
Served serve(std::vector<Client>* cs) {
  Served s;
  s.status.resize(cs->size());
  memset(s.status.data(), 0, cs->size() * sizeof(vpin_net_peer_status));
  std::vector<vpin_wire*> wires(cs->size());
  for (size_t i = 0; i < cs->size(); i++) {
    script(&(*cs)[i]);
    vpin_wire_io io{mem_send, mem_recv, &(*cs)[i]};
    CHECK(vpin_wire_create(&io, &wires[i]) == VPIN_OK);
  }
  Roster r;
  r.who = "multi_check"; r.max_batch = kMaxBatch; r.status = s.status.data();
  std::vector<std::vector<uint8_t>> last;  // per image slot, its last ciphertexts: c1 part, then c2 part
  for (size_t i = 0; i < cs->size(); i++) {
    std::vector<uint8_t> hello, input;
    size_t n = 0;
    bool told = false;
    const int rc = read_client(wires[i], kPer, kMaxBatch - r.images, &hello, &input, &n, &told);
    if (rc) {
      r.report(i, rc, VPIN_NET_STAGE_ADMISSION, vpin_last_error());
      if (!told) send_error(wires[i], rc, s.status[i].text);
      continue;
    }
    CHECK(hello.size() == 32 && input.size() == 64 * n * kPer);
    r.admit(wires[i], i, n);
    for (size_t b = 0; b < n; b++) {  // the image's c1 part and c2 part out of the frame
      std::vector<uint8_t> im(input.begin() + 32 * b * kPer, input.begin() + 32 * (b + 1) * kPer);
      im.insert(im.end(), input.begin() + 32 * (n + b) * kPer, input.begin() + 32 * (n + b + 1) * kPer);
      last.push_back(im);
    }
  }
  s.images = r.images;
  if (r.peers.empty()) s.rc = VPIN_ESHAPE;
  for (size_t round = 0; round < kRounds && !s.rc; round++) {
    const size_t n = kRoundN[round], B = r.images;
    std::vector<uint8_t> packed(64 * B * n), c1, c2, reply;
    for (size_t b = 0; b < B; b++) {
      layer(last[b], round, n, &c1, &c2);
      memcpy(&packed[32 * b * n], c1.data(), 32 * n);
      memcpy(&packed[32 * (B + b) * n], c2.data(), 32 * n);
    }
    s.rc = exchange(&r, (int)round, kRoundFlags[round], 0, packed.data(), n, &reply);
    if (!(kRoundFlags[round] & VPIN_LENET_REENCRYPT)) { CHECK(reply.empty()); continue; }
    CHECK(reply.size() == packed.size());
    for (const Peer& p : r.peers) {
      if (p.live) continue;  // gone: its images hold what the server sent
      for (size_t half = 0; half < 2; half++)
        CHECK(!memcmp(&reply[32 * (half * B + p.first) * n], &packed[32 * (half * B + p.first) * n], 32 * p.n * n));
      s.echoes++;
    }
    for (size_t b = 0; b < B; b++) {
      last[b].assign(reply.begin() + 32 * b * n, reply.begin() + 32 * (b + 1) * n);
      last[b].insert(last[b].end(), reply.begin() + 32 * (B + b) * n, reply.begin() + 32 * (B + b + 1) * n);
    }
  }
  if (!s.rc && !finish(&r)) s.rc = VPIN_ECOMM;
  for (vpin_wire* w : wires) vpin_wire_free(w);
  return s;
}

size_t g_runs = 0, g_drops = 0, g_alone = 0, g_echoes = 0;

// one roster: every status as the fail stages say, the slots in wire order, and every survivor's bytes those of itself alone
void check(std::vector<Client> cs) {
  Served s = serve(&cs);
  g_runs++;
  g_echoes += s.echoes;
  size_t first = 0, alive = 0, admitted_n = 0;
  for (size_t i = 0; i < cs.size(); i++) {
    int code, stage;
    bool admitted;
    expected(cs[i].fail, &code, &stage, &admitted);
    const vpin_net_peer_status& st = s.status[i];
    admitted_n += admitted ? 1 : 0;
    CHECK(st.code == code && st.stage == stage);  // the run goes on while anybody is live, so every failure is reached
    CHECK(st.first_image == (admitted ? first : 0) && st.n_images == (admitted ? cs[i].images : 0));
    CHECK((code == VPIN_OK) == (st.text[0] == 0));
    if (code) { g_drops++; CHECK(!strncmp(st.text, "multi_check: ", 13)); }
    if (admitted) first += cs[i].images;
    if (cs[i].fail == kNone) alive++;
  }
  CHECK(s.images == first);
  CHECK(s.rc == (admitted_n == 0 ? VPIN_ESHAPE : alive ? VPIN_OK : VPIN_ECOMM));
  for (size_t i = 0; i < cs.size(); i++) {
    if (cs[i].fail != kNone) continue;
    std::vector<Client> one(1, cs[i]);
    const Served a = serve(&one);
    CHECK(a.rc == VPIN_OK && a.status[0].code == VPIN_OK && a.status[0].first_image == 0);
    CHECK(one[0].out == cs[i].out && !cs[i].out.empty() && cs[i].pos == cs[i].in.size());
    g_alone++;
  }
}

void compositions() {
  const size_t before = g_runs;
  std::vector<Client> cs;
  for (size_t K = 1; K <= 3; K++) {
    size_t total = 1;
    for (size_t i = 0; i < K; i++) total *= 3;
    for (size_t code = 0; code < total; code++) {
      cs.assign(K, Client());
      size_t c = code;
      for (size_t i = 0; i < K; i++, c /= 3) { cs[i].id = 10 * K + i; cs[i].images = 1 + c % 3; }
      check(cs);
    }
  }
  uint64_t seed = 0x726f73746572;  // "roster"
  for (size_t K = 4; K <= 5; K++)
    for (int it = 0; it < 40; it++) {
      cs.assign(K, Client());
      for (size_t i = 0; i < K; i++) { cs[i].id = 100 * K + i; cs[i].images = 1 + splitmix(&seed) % 3; }
      check(cs);
    }
  printf("multi_check: %zu rosters of 1 .. 5 clients with 1 .. 3 images each, nobody dropped\n", g_runs - before);
}

void every_drop() {
  const size_t before = g_runs;
  uint64_t seed = 0x64726f70;  // "drop"
  for (size_t K = 1; K <= 5; K++)
    for (size_t who = 0; who < K; who++)
      for (int f = kFirstFrame; f < kFails; f++) {
        std::vector<Client> cs(K);
        for (size_t i = 0; i < K; i++) { cs[i].id = 1000 * K + i; cs[i].images = 1 + splitmix(&seed) % 3; }
        cs[who].fail = f;
        check(cs);
      }
  printf("multi_check: %zu rosters with one client dropped at each of %d stages in turn\n", g_runs - before, kFails - 1);
}

void random_drops() {
  const size_t before = g_runs;
  uint64_t seed = 0x72616e646f6d;  // "random"
  for (int it = 0; it < 2000;) {  // it counts the rosters checked
    const size_t K = 1 + splitmix(&seed) % 5;
    std::vector<Client> cs(K);
    for (size_t i = 0; i < K; i++) {
      cs[i].id = 7000 + 10 * (uint64_t)it + i;
      cs[i].images = 1 + splitmix(&seed) % 3;
      cs[i].fail = splitmix(&seed) % 2 ? kNone : 1 + (int)(splitmix(&seed) % (kFails - 1));
    }
    check(cs);
    it++;
  }
  printf("multi_check: %zu seeded rosters with random drops\n", g_runs - before);
}

}  // namespace

int main() {
  compositions();
  every_drop();
  random_drops();
  printf("multi_check: %zu rosters, %zu dropped clients, %zu rounds with a dropped client's images echoed, %zu survivors compared with themselves alone\n",
         g_runs, g_drops, g_echoes, g_alone);
  printf("multi_check: ok\n");
  return 0;
}
