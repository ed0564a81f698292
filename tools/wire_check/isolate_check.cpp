// isolate_check.cpp -- images and clients that leave a running batch, under the host compiler's sanitizers.  The slot
// bookkeeping of the isolated driver (vpin_amd/csrc/infer_slots.cpp) and the roster's positions (vpin_amd/csrc/wire_roster.cpp)
// decide whose bytes go where once the batch no longer holds everybody.  This program links them with wire_codec.cpp and
// wire_stream.cpp alone: no HIP, no Python, no GPU.  It is run by hand on a CPU machine and is part of no test suite.  From the
// repository's root:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//       tools/wire_check/isolate_check.cpp vpin_amd/csrc/wire_roster.cpp vpin_amd/csrc/wire_codec.cpp vpin_amd/csrc/wire_stream.cpp \
//       vpin_amd/csrc/infer_slots.cpp -o tools/wire_check/isolate_check && tools/wire_check/isolate_check
//
// (the clang++ of ROCm's LLVM serves).  As in multi_check.cpp the clients are scripts over vpin_wire_io callbacks in memory.  The
// server is the isolated endpoint's loop (wire_multi.cpp's multi_round around infer_core.cpp's run) with the device taken out: three
// "layers" with a round after each; a layer makes an image's next ciphertexts from that image's last ones and its SLOT's key alone,
// refuses the rows of the images that are planned to refuse, and is run again over the others; before a round the roster is
// re-based on the live slots and the clients that lost an image are dropped, after it the images of the clients that are gone
// leave.  It does three things and prints a line for each:
//   1. K = 1 .. 5 clients with B_i in 1 .. 3 images: each client in turn leaves at each layer (each of its images in turn
//      refused) and at each round (ERROR, a REPLY for another round, with another cnt, cut in half);
//   2. the same with a second client that leaves in the same step the other way (a refusal and a wire drop in one step), and
//      with one client that does both;
//   3. 3000 seeded rosters in which random subsets leave at random steps, by either way or both.
// In every run: each status names the code and the stage, the positions of the live clients are those of their slots among the
// live slots, the keys handed to a layer are the live slots', every survivor receives byte for byte what it receives in a roster
// that holds it alone in the same slots, and the run ends with VPIN_ECOMM when nobody is left.
// Exit status 0 and "isolate_check: ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vpin_amd/csrc/infer_slots.h"
#include "../../vpin_amd/csrc/wire.h"

// what the library defines over its own error text
static thread_local std::string g_error;
namespace vpin::wire {
void set_error(const char* text) { g_error = text; }
}  // namespace vpin::wire
extern "C" const char* vpin_last_error(void) { return g_error.c_str(); }

#define CHECK(cond)                                                                                      \
  do {                                                                                                   \
    if (!(cond)) {                                                                                       \
      fprintf(stderr, "isolate_check: %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, vpin_last_error()); \
      exit(1);                                                                                           \
    }                                                                                                    \
  } while (0)

using namespace vpin::wire;
using vpin::infer::Pts;
using vpin::infer::Slots;

namespace {

constexpr size_t kPer = 3, kSteps = 3, kMaxBatch = 15;
constexpr size_t kRoundN[kSteps] = {2, 3, 1};  // ciphertexts per image
constexpr int kRoundFlags[kSteps] = {VPIN_LENET_RELU | VPIN_LENET_REENCRYPT, VPIN_LENET_REENCRYPT, 0};
constexpr int kHows = 4;  // in a round: ERROR, a REPLY for another round, with another cnt, cut in half

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

// one client: who it is, its images, how it leaves; all it will ever send, all it is sent
struct Client {
  uint64_t id = 0;
  size_t images = 1;
  int refuse_layer = -1, refuse_image = 0;  // a layer refuses this image of its
  int fail_round = -1, how = 0;             // it fails on the wire in this round
  std::vector<uint8_t> in, out;
  size_t pos = 0;
  bool leaves() const { return refuse_layer >= 0 || fail_round >= 0; }
};

void script(Client* c) {
  std::vector<uint8_t> p;
  c->in.clear(); c->out.clear(); c->pos = 0;
  fill(&p, 32, c->id * 1000 + 1);
  append_frame(&c->in, VPIN_WIRE_HELLO, 0, 1, p);
  fill(&p, 64 * c->images * kPer, c->id * 1000 + 2);
  append_frame(&c->in, VPIN_WIRE_INPUT, 0, (uint32_t)(c->images * kPer), p);
  for (size_t r = 0; r < kSteps; r++) {
    const size_t cnt = (kRoundFlags[r] & VPIN_LENET_REENCRYPT) ? c->images * kRoundN[r] : 0;
    fill(&p, 64 * cnt, c->id * 1000 + 10 + r);
    if ((int)r != c->fail_round) { append_frame(&c->in, VPIN_WIRE_REPLY, (uint32_t)r, (uint32_t)cnt, p); continue; }
    if (c->how == 0) {
      append_frame(&c->in, VPIN_WIRE_ERROR, 0, 0, std::vector<uint8_t>{0xfb, 0xff, 0xff, 0xff, 'n', 'o'});
    } else if (c->how == 1) {
      append_frame(&c->in, VPIN_WIRE_REPLY, (uint32_t)r + 1, (uint32_t)cnt, p);
    } else if (c->how == 2) {
      fill(&p, 64 * (cnt + 1), 7);
      append_frame(&c->in, VPIN_WIRE_REPLY, (uint32_t)r, (uint32_t)cnt + 1, p);
    } else {
      append_frame(&c->in, VPIN_WIRE_REPLY, (uint32_t)r, (uint32_t)cnt, p, true);
    }
    return;
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

// what the client's status has to say: the first of its two ways out that the run reaches.  The refusal of layer L comes before
// the exchange of round L
void expected(const Client& c, int* code, int* stage) {
  *code = VPIN_OK; *stage = VPIN_NET_STAGE_DONE;
  if (c.refuse_layer >= 0 && (c.fail_round < 0 || c.refuse_layer <= c.fail_round)) { *code = VPIN_ESHAPE; *stage = VPIN_NET_STAGE_LAYER; return; }
  if (c.fail_round < 0) return;
  *stage = c.fail_round;
  *code = c.how == 1 || c.how == 2 ? VPIN_ESHAPE : VPIN_ECOMM;
}

// an image's next ciphertexts from its last ones and its slot's key alone: n points per half
void layer(const uint8_t* c1, const uint8_t* c2, size_t per, const uint8_t* key32, size_t step, size_t n, std::vector<uint8_t>* o1,
           std::vector<uint8_t>* o2) {
  uint64_t h = 0xcbf29ce484222325ull + step;
  for (size_t i = 0; i < 32 * per; i++) h = (h ^ c1[i]) * 0x100000001b3ull;
  for (size_t i = 0; i < 32 * per; i++) h = (h ^ c2[i]) * 0x100000001b3ull;
  for (size_t i = 0; i < 32; i++) h = (h ^ key32[i]) * 0x100000001b3ull;
  fill(o1, 32 * n, h);
  fill(o2, 32 * n, h ^ 0x5555);
}

struct Served {
  int rc = VPIN_OK;
  std::vector<vpin_net_peer_status> status;
  size_t repeats = 0, refused = 0, compacted = 0, rebased = 0;
};

// The isolated endpoint's loop without the device.  slot0: the clients' slots begin there (the slots before are nobody's and have
// left before the first layer): a client alone in the slots it had among others
Served serve(std::vector<Client>* cs, size_t slot0) {
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
  r.who = "isolate_check"; r.max_batch = kMaxBatch; r.status = s.status.data();
  r.images = slot0;
  Pts cur;  // the batch, position after position: x holds an image's c1 part, y its c2 part
  std::vector<int> refuse_at(kMaxBatch + 3, -1);  // per slot: the layer that refuses it
  for (size_t i = 0; i < cs->size(); i++) {
    std::vector<uint8_t> hello, input;
    size_t n = 0;
    bool told = false;
    CHECK(read_client(wires[i], kPer, kMaxBatch - r.images, &hello, &input, &n, &told) == VPIN_OK && n == (*cs)[i].images);
    if ((*cs)[i].refuse_layer >= 0) refuse_at[r.images + (size_t)(*cs)[i].refuse_image] = (*cs)[i].refuse_layer;
    r.admit(wires[i], i, n);
    const std::vector<uint8_t> flags(n * kPer, 0);
    cur.append(input.data(), input.data() + 32 * n * kPer, flags.data(), n * kPer);
  }
  const size_t B = r.images;
  std::vector<uint8_t> keys;  // slot-major: slot b's key of step L at 32 (b * kSteps + L)
  fill(&keys, 32 * B * kSteps, 0x6b657973);
  std::vector<vpin_net_image_status> image_status(B);
  memset(image_status.data(), 0, B * sizeof(vpin_net_image_status));
  Slots live(B);
  std::vector<size_t> nobody(slot0);
  for (size_t b = 0; b < slot0; b++) nobody[b] = b;
  live.remove(nobody);
  size_t per = kPer;
  for (size_t step = 0; step < kSteps && !s.rc; step++) {
    const size_t n = kRoundN[step];
    Pts next;
    for (;;) {  // the layer call, again without the images it refuses
      next.resize(0);
      std::vector<uint8_t> own, o1, o2;
      const uint8_t* k = vpin::infer::of_live_images(keys.data() + 32 * step, kSteps, 1, live, &own);
      std::vector<uint32_t> units;
      const std::vector<uint8_t> flags(n, 0);
      for (size_t at = 0; at < live.n(); at++) {
        CHECK(!memcmp(k + 32 * at, &keys[32 * (live.live[at] * kSteps + step)], 32));  // the key of the slot, not of the position
        layer(&cur.x[32 * at * per], &cur.y[32 * at * per], per, k + 32 * at, step, n, &o1, &o2);
        next.append(o1.data(), o2.data(), flags.data(), n);
        if (refuse_at[live.live[at]] == (int)step) { units.push_back((uint32_t)(2 * at)); units.push_back((uint32_t)(2 * at + 1)); }
      }
      if (units.empty()) break;
      const std::vector<size_t> gone = vpin::infer::positions_of_units(units.data(), units.size(), 2, live.n());
      CHECK(gone.size() * 2 == units.size());
      for (const size_t at : gone) {
        CHECK(refuse_at[live.live[at]] == (int)step);
        image_status[live.live[at]].code = VPIN_ESHAPE;
        snprintf(image_status[live.live[at]].text, sizeof image_status[0].text, "layer %zu refuses", step);
      }
      vpin::infer::remove_images(&cur, live.n(), gone);
      live.remove(gone);
      s.repeats++;
      if (!live.n()) break;
    }
    if (!live.n()) {  // the driver's "no image is left": whoever is still there is told the layer's text
      r.drop_refused(image_status.data());
      CHECK(!r.live());
      s.rc = VPIN_ECOMM;
      break;
    }
    CHECK(next.n() == live.n() * n && cur.n() == live.n() * per);
    // the round: where everybody stands now, who lost an image, the exchange over the batch at hand
    r.rebase(live.live.data(), live.n());
    s.refused += r.drop_refused(image_status.data());
    for (const Peer& p : r.peers) {
      if (!p.live) continue;
      CHECK(p.present == p.n && p.at + p.n <= live.n());
      for (size_t j = 0; j < p.n; j++) CHECK(live.live[p.at + j] == p.first + j);
      s.rebased++;
    }
    if (!r.live()) { s.rc = VPIN_ECOMM; break; }
    std::vector<uint8_t> packed(next.x), reply;
    packed.insert(packed.end(), next.y.begin(), next.y.end());
    s.rc = exchange(&r, (int)step, kRoundFlags[step], 0, packed.data(), n, &reply);
    if (s.rc) break;
    std::vector<size_t> away;
    for (const auto& g : r.gone(live.live.data())) {
      const vpin_net_peer_status& st = s.status[r.peers[g.first].wire];
      for (const uint32_t b : g.second) {
        CHECK(live.position(b) < live.n() && st.code != VPIN_OK);
        away.push_back(live.position(b));
        image_status[b].code = st.code;
      }
      if (st.stage != VPIN_NET_STAGE_LAYER) s.compacted += g.second.size();
    }
    std::sort(away.begin(), away.end());
    if (kRoundFlags[step] & VPIN_LENET_REENCRYPT) {
      CHECK(reply.size() == packed.size());
      next.x.assign(reply.begin(), reply.begin() + 32 * live.n() * n);
      next.y.assign(reply.begin() + 32 * live.n() * n, reply.end());
    }
    vpin::infer::remove_images(&next, live.n(), away);
    live.remove(away);
    cur = next;
    per = n;
    CHECK(live.n() && cur.n() == live.n() * per);  // exchange has seen that somebody is live
  }
  if (!s.rc && !finish(&r)) s.rc = VPIN_ECOMM;
  for (vpin_wire* w : wires) vpin_wire_free(w);
  return s;
}

size_t g_runs = 0, g_left = 0, g_alone = 0, g_repeats = 0, g_rebased = 0, g_nobody = 0, g_refused = 0, g_compacted = 0;

// one roster: every status as planned, every survivor's bytes those of itself alone in its slots, VPIN_ECOMM when nobody stays
void check(std::vector<Client> cs) {
  Served s = serve(&cs, 0);
  g_runs++;
  g_repeats += s.repeats; g_rebased += s.rebased; g_refused += s.refused; g_compacted += s.compacted;
  size_t first = 0, alive = 0;
  for (const Client& c : cs) alive += c.leaves() ? 0 : 1;
  for (size_t i = 0; i < cs.size(); i++) {
    int code, stage;
    expected(cs[i], &code, &stage);
    const vpin_net_peer_status& st = s.status[i];
    CHECK(st.first_image == first && st.n_images == cs[i].images);
    CHECK(st.code == code && st.stage == stage);  // the run goes on while anybody is live, so every way out is reached
    CHECK((code == VPIN_OK) == (st.text[0] == 0));
    if (code) g_left++;
    if (!cs[i].leaves()) {
      std::vector<Client> one(1, cs[i]);
      const Served a = serve(&one, first);
      CHECK(a.rc == VPIN_OK && a.status[0].code == VPIN_OK && a.status[0].first_image == first);
      CHECK(one[0].out == cs[i].out && !cs[i].out.empty() && cs[i].pos == cs[i].in.size());
      g_alone++;
    }
    first += cs[i].images;
  }
  CHECK(s.rc == (alive ? VPIN_OK : VPIN_ECOMM));
  if (!alive) g_nobody++;
}

std::vector<Client> roster(size_t K, uint64_t* seed, uint64_t id0) {
  std::vector<Client> cs(K);
  for (size_t i = 0; i < K; i++) { cs[i].id = id0 + i; cs[i].images = 1 + splitmix(seed) % 3; }
  return cs;
}

void each_in_turn() {
  const size_t before = g_runs;
  uint64_t seed = 0x7475726e;  // "turn"
  for (size_t K = 1; K <= 5; K++)
    for (size_t who = 0; who < K; who++)
      for (size_t step = 0; step < kSteps; step++) {
        for (int how = 0; how < kHows; how++) {
          std::vector<Client> cs = roster(K, &seed, 1000 * K);
          cs[who].fail_round = (int)step; cs[who].how = how;
          check(cs);
        }
        for (size_t im = 0; im < 3; im++) {
          std::vector<Client> cs = roster(K, &seed, 2000 * K);
          if (im >= cs[who].images) continue;
          cs[who].refuse_layer = (int)step; cs[who].refuse_image = (int)im;
          check(cs);
        }
      }
  printf("isolate_check: %zu rosters with one client leaving at each layer and each round in turn\n", g_runs - before);
}

void both_in_one_step() {
  const size_t before = g_runs;
  uint64_t seed = 0x626f7468;  // "both"
  for (size_t K = 1; K <= 5; K++)
    for (size_t who = 0; who < K; who++)
      for (size_t other = 0; other < K; other++)
        for (size_t step = 0; step < kSteps; step++)
          for (int how = 0; how < kHows; how++) {
            std::vector<Client> cs = roster(K, &seed, 3000 * K);
            cs[who].refuse_layer = (int)step; cs[who].refuse_image = (int)(splitmix(&seed) % cs[who].images);
            cs[other].fail_round = (int)step; cs[other].how = how;  // other == who: one client does both
            check(cs);
          }
  printf("isolate_check: %zu rosters with a refusal and a wire drop in the same step\n", g_runs - before);
}

void random_subsets() {
  const size_t before = g_runs;
  uint64_t seed = 0x73756273657473;  // "subsets"
  for (int it = 0; it < 3000; it++) {
    const size_t K = 1 + splitmix(&seed) % 5;
    std::vector<Client> cs = roster(K, &seed, 9000 + 10 * (uint64_t)it);
    for (Client& c : cs) {
      const uint64_t way = splitmix(&seed) % 5;  // 0, 1: stays; 2: refused; 3: wire; 4: both
      if (way == 2 || way == 4) { c.refuse_layer = (int)(splitmix(&seed) % kSteps); c.refuse_image = (int)(splitmix(&seed) % c.images); }
      if (way == 3 || way == 4) { c.fail_round = (int)(splitmix(&seed) % kSteps); c.how = (int)(splitmix(&seed) % kHows); }
    }
    check(cs);
  }
  printf("isolate_check: %zu seeded rosters with random subsets leaving at random steps\n", g_runs - before);
}

}  // namespace

int main() {
  each_in_turn();
  both_in_one_step();
  random_subsets();
  printf("isolate_check: %zu rosters, %zu clients that left (%zu images with a refused client, %zu images compacted away), %zu layer calls repeated, "
         "%zu positions re-based and compared, %zu runs that nobody finished, %zu survivors compared with themselves alone\n",
         g_runs, g_left, g_refused, g_compacted, g_repeats, g_rebased, g_nobody, g_alone);
  printf("isolate_check: ok\n");
  return 0;
}
