// wire_roster.cpp -- several clients in one batched inference: who gets which bytes.  The roster gives the admitted clients
// their image slots in wire order, cuts each client's frame out of a packed round, puts a reply's points back into the batch,
// and leaves a dropped client's images what the server sent; it reads a client's HELLO and INPUT and runs one round's exchange
// with all live clients.  For the isolated server it re-bases every client's position on the slots still in the batch, drops
// the clients that lost an image to a layer and names the images of the clients that are gone (tools/wire_check/isolate_check.cpp).  Plain C++ beside wire_codec.cpp and wire_stream.cpp: no HIP, no context.  It decides which client's
// bytes go where and parses what untrusted peers send, so tools/wire_check/multi_check.cpp links these three files alone and
// runs them under the host compiler's sanitizers.  wire_multi.cpp is the endpoint around it.
#include <cstdio>
#include <cstring>

#include "wire.h"

namespace vpin::wire {

size_t Roster::live() const {
  size_t n = 0;
  for (const Peer& p : peers) n += p.live ? 1 : 0;
  return n;
}

void Roster::admit(vpin_wire* w, size_t wire, size_t n_images) {
  Peer p;
  p.w = w; p.wire = wire; p.first = p.at = images; p.n = p.present = n_images;
  images += n_images;
  batch = images;
  peers.push_back(p);
  status[wire].first_image = (uint32_t)p.first;
  status[wire].n_images = (uint32_t)p.n;
}

void Roster::report(size_t wire, int code, int stage, const std::string& text) {
  vpin_net_peer_status& s = status[wire];
  s.code = code;
  s.stage = stage;
  snprintf(s.text, sizeof s.text, "%s%s%s", code ? who : "", code ? ": " : "", text.c_str());
}

void Roster::drop(size_t p, int code, int stage, const std::string& text, bool tell) {
  peers[p].live = false;
  report(peers[p].wire, code, stage, text);
  if (tell) send_error(peers[p].w, code, status[peers[p].wire].text);
}

void Roster::rebase(const uint32_t* slots, size_t n) {
  size_t i = 0;
  for (Peer& p : peers) {
    while (i < n && slots[i] < p.first) i++;
    p.at = i;
    while (i < n && slots[i] < p.first + p.n) i++;
    p.present = i - p.at;
  }
  batch = n;
}

size_t Roster::drop_refused(const vpin_net_image_status* image_status) {
  size_t images_gone = 0;
  for (size_t i = 0; i < peers.size(); i++) {
    const Peer& p = peers[i];
    if (!p.live) continue;
    const vpin_net_image_status* why = nullptr;  // its first image that left
    for (size_t b = p.first; b < p.first + p.n && !why; b++)
      if (image_status[b].code) why = &image_status[b];
    if (!why) continue;
    images_gone += p.n;
    drop(i, why->code, VPIN_NET_STAGE_LAYER, why->text);
  }
  return images_gone;
}

std::vector<std::pair<size_t, std::vector<uint32_t>>> Roster::gone(const uint32_t* slots) const {
  std::vector<std::pair<size_t, std::vector<uint32_t>>> out;
  for (size_t i = 0; i < peers.size(); i++) {
    const Peer& p = peers[i];
    if (p.live || !p.present) continue;
    out.emplace_back(i, std::vector<uint32_t>(slots + p.at, slots + p.at + p.present));
  }
  return out;
}

void slice(const Roster& r, const Peer& p, const uint8_t* packed, size_t per, std::vector<uint8_t>* frame) {
  const size_t part = 32 * p.present * per, c2 = 32 * r.batch * per;
  frame->resize(2 * part);
  memcpy(frame->data(), packed + 32 * p.at * per, part);
  memcpy(frame->data() + part, packed + c2 + 32 * p.at * per, part);
}

void place(const Roster& r, const Peer& p, const uint8_t* frame, size_t per, uint8_t* packed) {
  const size_t part = 32 * p.present * per, c2 = 32 * r.batch * per;
  memcpy(packed + 32 * p.at * per, frame, part);
  memcpy(packed + c2 + 32 * p.at * per, frame + part, part);
}

void copy_images(const Peer& p, size_t per, size_t elem, const uint8_t* from, uint8_t* to) {
  memcpy(to + elem * p.at * per, from + elem * p.at * per, elem * p.present * per);
}

int read_client(vpin_wire* w, size_t per, size_t room, std::vector<uint8_t>* hello, std::vector<uint8_t>* input,
                size_t* n_images, bool* told) {
  char why[240];
  vpin_wire_header h;
  *told = false;
  *n_images = 0;
  int rc = recv_header(w, &h);
  if (rc) return rc;
  if (h.type == VPIN_WIRE_ERROR) { *told = true; return peer_error(w, h, "the client"); }
  if (h.type != VPIN_WIRE_HELLO) {
    snprintf(why, sizeof why, "expected HELLO, the peer sent type %u", (unsigned)h.type);
    return fail(VPIN_ESHAPE, why);
  }
  Lap lap;
  rc = recv_payload(w, h, hello);
  add_ms(w, 0, kRecv, lap());
  if (rc) return rc;
  if ((rc = recv_header(w, &h))) return rc;
  if (h.type == VPIN_WIRE_ERROR) { *told = true; return peer_error(w, h, "the client"); }
  if (h.type != VPIN_WIRE_INPUT) {
    snprintf(why, sizeof why, "expected INPUT, the peer sent type %u with cnt %u", (unsigned)h.type, (unsigned)h.cnt);
    return fail(VPIN_ESHAPE, why);
  }
  if (!h.cnt || h.cnt % per) {
    snprintf(why, sizeof why, "expected INPUT of whole images of %zu ciphertexts, the peer sent cnt %u", per, (unsigned)h.cnt);
    return fail(VPIN_ESHAPE, why);
  }
  if (h.cnt / per > room) {
    snprintf(why, sizeof why, "the peer sent %zu images, the batch has room for %zu more", (size_t)h.cnt / per, room);
    return fail(VPIN_ESHAPE, why);
  }
  lap();
  rc = recv_payload(w, h, input);
  add_ms(w, 0, kRecv, lap());
  if (rc) return rc;
  *n_images = h.cnt / per;
  return VPIN_OK;
}

int exchange(Roster* r, int round, int flags, int shift_bits, const uint8_t* packed, size_t per, std::vector<uint8_t>* reply) {
  const bool re = (flags & VPIN_LENET_REENCRYPT) != 0;
  const size_t slot = 1 + (size_t)round;
  const std::string at = "round " + std::to_string(round) + ": ";
  char why[240];
  reply->clear();
  if (re) reply->assign(packed, packed + 64 * r->batch * per);  // the places of a client that is not live: what the server sent
  std::vector<uint8_t> frame;
  for (size_t i = 0; i < r->peers.size(); i++) {
    Peer& p = r->peers[i];
    if (!p.live) continue;
    slice(*r, p, packed, per, &frame);
    vpin_wire_header h;
    memset(&h, 0, sizeof h);
    h.type = VPIN_WIRE_ROUND; h.flags = (uint8_t)flags; h.shift_bits = (uint8_t)shift_bits;
    h.round = (uint32_t)round; h.cnt = (uint32_t)(p.n * per); h.payload_len = frame.size();
    Lap lap;
    const int rc = send_frame(p.w, h, frame.data());
    add_ms(p.w, slot, kSend, lap());
    if (rc) r->drop(i, rc, round, at + vpin_last_error());
  }
  for (size_t i = 0; i < r->peers.size(); i++) {
    Peer& p = r->peers[i];
    if (!p.live) continue;
    const size_t cnt = p.n * per, want = re ? cnt : 0;
    vpin_wire_header h;
    int rc = recv_header(p.w, &h);
    if (rc) { r->drop(i, rc, round, at + vpin_last_error()); continue; }
    if (h.type == VPIN_WIRE_ERROR) {
      rc = peer_error(p.w, h, "the client");
      r->drop(i, rc, round, at + vpin_last_error(), false);
      continue;
    }
    if (h.type != VPIN_WIRE_REPLY) {
      snprintf(why, sizeof why, "expected REPLY, the peer sent type %u", (unsigned)h.type);
      r->drop(i, VPIN_ESHAPE, round, at + why);
      continue;
    }
    if (h.round != (uint32_t)round) {
      snprintf(why, sizeof why, "the reply is for round %u", (unsigned)h.round);
      r->drop(i, VPIN_ESHAPE, round, at + why);
      continue;
    }
    if (h.cnt != want) {
      snprintf(why, sizeof why, "the reply holds %u ciphertexts, the round asked for %zu", (unsigned)h.cnt, want);
      r->drop(i, VPIN_ESHAPE, round, at + why);
      continue;
    }
    Lap lap;
    rc = recv_payload(p.w, h, &frame);
    add_ms(p.w, slot, kRecv, lap());
    if (rc) { r->drop(i, rc, round, at + vpin_last_error()); continue; }
    if (re) place(*r, p, frame.data(), per, reply->data());
  }
  if (!r->live()) return fail(VPIN_ECOMM, (std::string(r->who) + ": " + at + "no client is left").c_str());
  return VPIN_OK;
}

size_t finish(Roster* r) {
  size_t told = 0;
  vpin_wire_header h;
  memset(&h, 0, sizeof h);
  h.type = VPIN_WIRE_DONE;
  for (size_t i = 0; i < r->peers.size(); i++) {
    Peer& p = r->peers[i];
    if (!p.live) continue;
    const int rc = send_frame(p.w, h, nullptr);
    if (rc) { r->drop(i, rc, VPIN_NET_STAGE_DONE, std::string("DONE: ") + vpin_last_error(), false); continue; }
    r->report(p.wire, VPIN_OK, VPIN_NET_STAGE_DONE, "");
    told++;
  }
  return told;
}

}  // namespace vpin::wire
