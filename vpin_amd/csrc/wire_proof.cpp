// wire_proof.cpp -- the proof records that follow DONE on the inference stream (include/vpin_hip.h has the layout): the 40-byte
// header encoded and decoded, one record sent and received over a vpin_wire, and the client's receiving state machine, which
// takes from the stream exactly the records its own expectation lists.  Plain C++ beside wire_codec.cpp and wire_stream.cpp: the
// bytes come from an untrusted peer, and tools/wire_check/proof_check.cpp runs this file under the host compiler's sanitizers.
// What a header may make a receiver allocate is bounded by the shape (is_mult, n_ops) it names: host/proof_sizes.h.
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "host/proof_sizes.h"
#include "wire.h"

namespace vpin::wire {

namespace {

const uint8_t kMagic[4] = {'V', 'P', 'P', '1'};

void put_le(uint8_t* p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}
uint64_t get_le(const uint8_t* p, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

// the rules both directions share; who: the entry point the text names
int check(const vpin_proof_header& h, const char* who) {
  char why[200];
  auto no = [&](const char* rule) {
    snprintf(why, sizeof why, "%s: %s", who, rule);
    return fail(VPIN_EINVAL, why);
  };
  if (h.kind < VPIN_PROOF_RECORD || h.kind > VPIN_PROOF_ERROR) {
    snprintf(why, sizeof why, "%s: unknown kind %u", who, (unsigned)h.kind);
    return fail(VPIN_EINVAL, why);
  }
  if (h.kind == VPIN_PROOF_END) {
    if (h.is_mult || h.label || h.n_ops || h.proof_len || h.comm_len) return no("END: a field that must be zero is not");
    return VPIN_OK;
  }
  if (h.kind == VPIN_PROOF_ERROR) {
    if (h.is_mult || h.image || h.label || h.n_ops || h.comm_len) return no("ERROR: a field that must be zero is not");
    if (h.proof_len < 4 || h.proof_len > 4 + VPIN_WIRE_MAX_TEXT) {
      snprintf(why, sizeof why, "%s: ERROR: proof_len %llu is outside 4 .. 4 + VPIN_WIRE_MAX_TEXT", who, (unsigned long long)h.proof_len);
      return fail(VPIN_EINVAL, why);
    }
    return VPIN_OK;
  }
  if (h.is_mult > 1) {
    snprintf(why, sizeof why, "%s: is_mult %u is above 1", who, (unsigned)h.is_mult);
    return fail(VPIN_EINVAL, why);
  }
  if (h.n_ops == 0 || h.n_ops > VPIN_PROOF_MAX_OPS) {
    snprintf(why, sizeof why, "%s: n_ops %llu is outside 1 .. VPIN_PROOF_MAX_OPS", who, (unsigned long long)h.n_ops);
    return fail(VPIN_EINVAL, why);
  }
  const uint64_t cap = vpin_gadget_proof_max_bytes(h.is_mult, (size_t)h.n_ops), comm = vpin_gadget_comm_bytes(h.is_mult, (size_t)h.n_ops);
  if (h.proof_len > cap) {
    snprintf(why, sizeof why, "%s: proof_len %llu is above the %llu bytes a proof of %llu %s can take", who, (unsigned long long)h.proof_len,
             (unsigned long long)cap, (unsigned long long)h.n_ops, h.is_mult ? "multiplications" : "additions");
    return fail(VPIN_EINVAL, why);
  }
  if (h.comm_len != comm) {
    snprintf(why, sizeof why, "%s: comm_len %llu is not the %llu bytes of the commitment of %llu %s", who, (unsigned long long)h.comm_len,
             (unsigned long long)comm, (unsigned long long)h.n_ops, h.is_mult ? "multiplications" : "additions");
    return fail(VPIN_EINVAL, why);
  }
  return VPIN_OK;
}

uint64_t payload_len(const vpin_proof_header& h) {
  if (h.kind == VPIN_PROOF_ERROR) return h.proof_len;
  if (h.kind != VPIN_PROOF_RECORD) return 0;
  return h.proof_len + h.comm_len + 64 * (uint64_t)vpin_gadget_vars_rows(h.is_mult, (size_t)h.n_ops);
}

const char* ops_name(int is_mult) { return is_mult ? "multiplications" : "additions"; }

}  // namespace

int send_proof(vpin_wire* w, const vpin_proof_header& h, const void* payload) {
  uint8_t head[VPIN_PROOF_HEADER_LEN];
  int rc = vpin_proof_header_encode(&h, head);
  if (rc) return rc;
  const uint64_t n = payload_len(h);
  if (n && !payload) return fail(VPIN_EINVAL, "vpin_proof_send: the record has a payload and none is given");
  if ((rc = send_all(w, head, sizeof head))) return rc;
  if ((rc = send_all(w, payload, (size_t)n))) return rc;
  w->stats[2]++;
  return VPIN_OK;
}

int recv_proof_header(vpin_wire* w, vpin_proof_header* h) {
  uint8_t head[VPIN_PROOF_HEADER_LEN];
  int rc = recv_all(w, head, sizeof head);
  if (rc) return rc;
  if ((rc = vpin_proof_header_decode(head, h))) return rc;
  if (!payload_len(*h)) w->stats[3]++;  // the whole record; one with a payload counts once that is in
  return VPIN_OK;
}

void send_proof_error(vpin_wire* w, int code, const char* text) {
  char keep[VPIN_WIRE_MAX_TEXT + 1];
  snprintf(keep, sizeof keep, "%s", vpin_last_error());
  uint8_t payload[4 + VPIN_WIRE_MAX_TEXT];
  const size_t n = strnlen(text ? text : "", VPIN_WIRE_MAX_TEXT);
  put_le(payload, (uint32_t)(int32_t)code, 4);
  memcpy(payload + 4, text ? text : "", n);
  vpin_proof_header h;
  memset(&h, 0, sizeof h);
  h.kind = VPIN_PROOF_ERROR;
  h.proof_len = 4 + n;
  (void)send_proof(w, h, payload);
  set_error(keep);
}

int recv_proofs(vpin_wire* w, const char* who, size_t n_images, const vpin_proof_expect* expect, size_t n_expect,
                std::vector<ProofRecord>* out, double* ms_recv) {
  char why[VPIN_WIRE_MAX_TEXT + 160];
  const size_t total = n_images * n_expect;
  Lap lap;
  auto done = [&](int rc) {
    if (ms_recv) *ms_recv += lap();
    return rc;
  };
  // refused before the payload is read: the peer is told, and the stream is of no more use
  auto refuse = [&]() {
    const std::string text = why;
    send_proof_error(w, VPIN_ESHAPE, text.c_str());
    return done(fail(VPIN_ESHAPE, text.c_str()));
  };
  out->clear();
  for (;;) {
    const size_t at = out->size();
    vpin_proof_header h;
    int rc = recv_proof_header(w, &h);
    if (rc) {
      const std::string text = std::string(who) + ": " + vpin_last_error();
      if (rc != VPIN_ECOMM) send_proof_error(w, rc, text.c_str());
      return done(fail(rc, text.c_str()));
    }
    if (h.kind == VPIN_PROOF_ERROR) {
      uint8_t p[4 + VPIN_WIRE_MAX_TEXT];
      if ((rc = recv_all(w, p, (size_t)h.proof_len))) return done(fail(rc, (std::string(who) + ": " + vpin_last_error()).c_str()));
      w->stats[3]++;
      snprintf(why, sizeof why, "%s: the peer reported an error (%d): %.*s", who, (int)(int32_t)(uint32_t)get_le(p, 4), (int)(h.proof_len - 4),
               (const char*)p + 4);
      return done(fail(VPIN_ECOMM, why));
    }
    if (h.kind == VPIN_PROOF_END) {
      if (at != total) {
        snprintf(why, sizeof why, "%s: the server ends after %zu of %zu proofs", who, at, total);
        return refuse();
      }
      if (h.image != total) {
        snprintf(why, sizeof why, "%s: the server's END counts %u proofs, %zu were sent", who, (unsigned)h.image, total);
        return refuse();
      }
      return done(VPIN_OK);
    }
    if (at == total) {
      snprintf(why, sizeof why, "%s: the server sends a proof behind the %zu the expectation lists", who, total);
      return refuse();
    }
    const size_t image = at / n_expect;
    const vpin_proof_expect& e = expect[at % n_expect];
    if (h.image != image || h.label != e.label) {
      snprintf(why, sizeof why, "%s: the server sends image %u, label %u, the expectation says image %zu, label %u comes next", who,
               (unsigned)h.image, (unsigned)h.label, image, (unsigned)e.label);
      return refuse();
    }
    if ((h.is_mult != 0) != (e.is_mult != 0) || h.n_ops != e.n_ops) {
      snprintf(why, sizeof why, "%s: image %zu, label %u: the server proves %llu %s, the expectation says %llu%s%s", who, image, (unsigned)e.label,
               (unsigned long long)h.n_ops, ops_name(h.is_mult), (unsigned long long)e.n_ops,
               (h.is_mult != 0) != (e.is_mult != 0) ? " " : "", (h.is_mult != 0) != (e.is_mult != 0) ? ops_name(e.is_mult) : "");
      return refuse();
    }
    try {
      out->emplace_back();
      out->back().h = h;
      out->back().payload.resize((size_t)payload_len(h));  // bounded by the shape the expectation names: decode has accepted the header
    } catch (const std::bad_alloc&) {
      return done(fail(VPIN_ENOMEM, (std::string(who) + ": no memory for the record").c_str()));
    }
    if ((rc = recv_all(w, out->back().payload.data(), out->back().payload.size()))) {
      out->pop_back();
      return done(fail(rc, (std::string(who) + ": " + vpin_last_error()).c_str()));
    }
    w->stats[3]++;
  }
}

}  // namespace vpin::wire

using namespace vpin::wire;

extern "C" {

size_t vpin_gadget_proof_max_bytes(int is_mult, size_t n_ops) {
  size_t nc, nv, nnz[3];
  vpin_sizes::gadget_dims(is_mult, n_ops, &nc, &nv, nnz);
  return vpin_sizes::snark_proof_max_bytes(nc, nv, nnz);
}

size_t vpin_gadget_comm_bytes(int is_mult, size_t n_ops) {
  size_t nc, nv, nnz[3];
  vpin_sizes::gadget_dims(is_mult, n_ops, &nc, &nv, nnz);
  return vpin_sizes::spark_comm_bytes(nc, nv, nnz);
}

size_t vpin_gadget_vars_rows(int is_mult, size_t n_ops) {
  size_t nc, nv, nnz[3];
  vpin_sizes::gadget_dims(is_mult, n_ops, &nc, &nv, nnz);
  return vpin_sizes::vars_rows(nv);
}

int vpin_proof_header_encode(const vpin_proof_header* h, uint8_t out40[VPIN_PROOF_HEADER_LEN]) {
  if (!h || !out40) return fail(VPIN_EINVAL, "vpin_proof_header_encode: null argument");
  const int rc = check(*h, "vpin_proof_header_encode");
  if (rc) return rc;
  memcpy(out40, kMagic, 4);
  out40[4] = h->kind; out40[5] = h->is_mult; out40[6] = 0; out40[7] = 0;
  put_le(out40 + 8, h->image, 4);
  put_le(out40 + 12, h->label, 4);
  put_le(out40 + 16, h->n_ops, 8);
  put_le(out40 + 24, h->proof_len, 8);
  put_le(out40 + 32, h->comm_len, 8);
  return VPIN_OK;
}

int vpin_proof_header_decode(const uint8_t in40[VPIN_PROOF_HEADER_LEN], vpin_proof_header* h) {
  if (!in40 || !h) return fail(VPIN_EINVAL, "vpin_proof_header_decode: null argument");
  if (memcmp(in40, kMagic, 4)) return fail(VPIN_EINVAL, "vpin_proof_header_decode: wrong magic");
  vpin_proof_header t;
  memset(&t, 0, sizeof t);
  t.kind = in40[4]; t.is_mult = in40[5];
  t.image = (uint32_t)get_le(in40 + 8, 4);
  t.label = (uint32_t)get_le(in40 + 12, 4);
  t.n_ops = get_le(in40 + 16, 8);
  t.proof_len = get_le(in40 + 24, 8);
  t.comm_len = get_le(in40 + 32, 8);
  if (t.kind < VPIN_PROOF_RECORD || t.kind > VPIN_PROOF_ERROR) return check(t, "vpin_proof_header_decode");  // unknown kind
  if (in40[6] || in40[7]) return fail(VPIN_EINVAL, "vpin_proof_header_decode: the reserved bytes are not zero");
  const int rc = check(t, "vpin_proof_header_decode");
  if (rc) return rc;
  *h = t;
  return VPIN_OK;
}

uint64_t vpin_proof_payload_len(const vpin_proof_header* h) { return h ? payload_len(*h) : 0; }

int vpin_proof_send(vpin_wire* w, const vpin_proof_header* h, const uint8_t* payload) {
  if (!w || !h) return fail(VPIN_EINVAL, "vpin_proof_send: null argument");
  return send_proof(w, *h, payload);
}

int vpin_proof_recv(vpin_wire* w, vpin_proof_header* h, uint8_t* payload, size_t cap) {
  if (!w || !h || (!payload && cap)) return fail(VPIN_EINVAL, "vpin_proof_recv: null argument");
  int rc = recv_proof_header(w, h);
  if (rc) return rc;
  const uint64_t n = payload_len(*h);
  if (n > cap) return fail(VPIN_EINVAL, "vpin_proof_recv: the record's payload is longer than the buffer");
  if ((rc = recv_all(w, payload, (size_t)n))) return rc;
  if (n) w->stats[3]++;
  return VPIN_OK;
}

}  // extern "C"
