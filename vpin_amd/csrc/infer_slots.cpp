// infer_slots.cpp -- which images are still in a running batch and what of the batch's arrays is theirs (infer_slots.h): the
// slots and their positions, a layer's refused units as positions, images cut out of the points the driver holds, and the keys
// and bias r of the live slots.  Plain C++: what vpin_net_infer_isolated (infer_core.cpp) does when a layer refuses or a round
// drops an image is decided here, away from the device.
#include "infer_slots.h"

#include <algorithm>
#include <cstring>

namespace vpin::infer {

Slots::Slots(size_t B) : live(B) {
  for (size_t b = 0; b < B; b++) live[b] = (uint32_t)b;
}

size_t Slots::position(uint32_t slot) const {
  const auto it = std::lower_bound(live.begin(), live.end(), slot);
  return it != live.end() && *it == slot ? (size_t)(it - live.begin()) : live.size();
}

void Slots::remove(const std::vector<size_t>& positions) {
  size_t next = 0, kept = 0;
  for (size_t i = 0; i < live.size(); i++) {
    if (next < positions.size() && positions[next] == i) { next++; continue; }
    live[kept++] = live[i];
  }
  live.resize(kept);
}

std::vector<size_t> positions_of_units(const uint32_t* units, size_t n_units, size_t per_image, size_t n) {
  std::vector<size_t> out;
  if (!per_image) return out;
  for (size_t i = 0; i < n_units; i++) {
    const size_t at = units[i] / per_image;
    if (at >= n) return {};
    if (out.empty() || out.back() != at) out.push_back(at);
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return out;
}

void remove_images(Pts* p, size_t n, const std::vector<size_t>& positions) {
  if (!n || positions.empty()) return;
  const size_t per = p->n() / n;
  size_t next = 0, kept = 0;
  for (size_t i = 0; i < n; i++) {
    if (next < positions.size() && positions[next] == i) { next++; continue; }
    if (kept != i) {
      memmove(&p->x[32 * kept * per], &p->x[32 * i * per], 32 * per);
      memmove(&p->y[32 * kept * per], &p->y[32 * i * per], 32 * per);
      memmove(&p->inf[kept * per], &p->inf[i * per], per);
    }
    kept++;
  }
  p->resize(kept * per);
}

const uint8_t* of_live_images(const uint8_t* at, size_t stride, size_t count, const Slots& s, std::vector<uint8_t>* own) {
  if (!count || !s.n()) return at;
  if (s.n() == 1) return at + 32 * stride * s.live[0];
  own->resize(32 * count * s.n());
  for (size_t i = 0; i < s.n(); i++) memcpy(own->data() + 32 * count * i, at + 32 * stride * s.live[i], 32 * count);
  return own->data();
}

}  // namespace vpin::infer
