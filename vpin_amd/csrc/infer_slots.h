// infer_slots.h -- the bookkeeping of images that leave a running batch (infer_slots.cpp; plain C++ like wire_roster.cpp: no
// HIP, no context, so tools/wire_check links it under the host compiler's sanitizers).  An image is named by its SLOT, its index
// in the batch the caller handed in, for its whole life: keys, bias r and public keys stay indexed by slot.  Its POSITION is its
// index among the images still there, in slot order; what the driver holds (c1, c2, a layer call's planes) is laid out by position.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vpin::infer {

// points as canonical little-endian bytes with a flag byte each
struct Pts {
  std::vector<uint8_t> x, y, inf;
  size_t n() const { return inf.size(); }
  void resize(size_t k) { x.resize(32 * k); y.resize(32 * k); inf.resize(k); }
  void append(const uint8_t* px, const uint8_t* py, const uint8_t* pf, size_t k) {
    x.insert(x.end(), px, px + 32 * k); y.insert(y.end(), py, py + 32 * k); inf.insert(inf.end(), pf, pf + k);
  }
  void append(const Pts& o, size_t from, size_t k) { append(o.x.data() + 32 * from, o.y.data() + 32 * from, o.inf.data() + from, k); }
};

// the slots still in the batch, ascending
struct Slots {
  std::vector<uint32_t> live;
  explicit Slots(size_t B = 0);
  size_t n() const { return live.size(); }
  bool whole(size_t B) const { return live.size() == B; }  // nobody has left: position = slot
  // the position of `slot`, or n() when it has left
  size_t position(uint32_t slot) const;
  // the images at these positions (ascending, no duplicates, all below n()) leave
  void remove(const std::vector<size_t>& positions);
};

// The units a layer call over n images refuses (vpin_enc_last_refusals: ascending) as positions, ascending without duplicates.
// An image's units stand together under both plane orders, Step::kBlocked and Step::kInterleaved, which only permute the planes
// INSIDE an image: per_image = 2 C * repeat planes for a convolution behind its channel sums and its repeat, 2 C for a pooling,
// 2 groups for a trained convolution, 2 rows for a fully connected layer.  Empty when a unit lies outside n * per_image
std::vector<size_t> positions_of_units(const uint32_t* units, size_t n_units, size_t per_image, size_t n);

// p holds n equal parts, one per position: those at `positions` (as for Slots::remove) go
void remove_images(Pts* p, size_t n, const std::vector<size_t>& positions);

// a step's `count` 32-byte items (PRF keys, bias r) of the live images, position after position: slot s's stand at
// at + 32 (s * stride + ..).  `own` holds them when they have to be put together
const uint8_t* of_live_images(const uint8_t* at, size_t stride, size_t count, const Slots& s, std::vector<uint8_t>* own);

}  // namespace vpin::infer
