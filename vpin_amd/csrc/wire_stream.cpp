// wire_stream.cpp -- frames over a transport of the caller's, and the transport over two descriptors (pipes, socketpairs,
// connected sockets).  Plain C++ beside wire_codec.cpp: no HIP, no context.  The descriptor form never blocks past its time-out
// (every read and write comes after a poll, writes to a pipe in pieces a ready pipe takes whole), retries EINTR, and turns
// end-of-file, a time-out and a write error into VPIN_ECOMM with a text; a closed peer never raises SIGPIPE (MSG_NOSIGNAL on a
// socket; elsewhere the signal is blocked around the write and a pending one is taken off before it is unblocked).
#include <cerrno>
#include <csignal>
#include <cstdio>
#include <cstring>
#include <new>

#include <poll.h>
#include <pthread.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <unistd.h>

#include "wire.h"

namespace vpin::wire {

namespace {

constexpr size_t kPipePiece = 4096;  // PIPE_BUF on Linux: a pipe that polls writable takes this much without blocking

// wait until fd is ready for `events`; 0, or VPIN_ECOMM with what was moved so far
int wait_fd(const vpin_wire* w, int fd, short events, const char* what, size_t done, size_t n) {
  char why[160];
  for (;;) {
    struct pollfd p = {fd, events, 0};
    const int rc = poll(&p, 1, w->timeout_ms);
    if (rc > 0) return VPIN_OK;  // ready, or hung up / in error: the read or write that follows says which
    if (rc == 0) {
      snprintf(why, sizeof why, "vpin_wire: timed out after %d ms %s, after %zu of %zu bytes", w->timeout_ms, what, done, n);
      return fail(VPIN_ECOMM, why);
    }
    if (errno == EINTR) continue;
    snprintf(why, sizeof why, "vpin_wire: poll failed %s: %s", what, strerror(errno));
    return fail(VPIN_ECOMM, why);
  }
}

// write to something that is not a socket with SIGPIPE kept from the process
ssize_t write_masked(int fd, const void* p, size_t n) {
  sigset_t pipe_set, old, pending;
  sigemptyset(&pipe_set);
  sigaddset(&pipe_set, SIGPIPE);
  sigpending(&pending);
  const bool was_pending = sigismember(&pending, SIGPIPE) == 1;
  pthread_sigmask(SIG_BLOCK, &pipe_set, &old);
  const ssize_t rc = write(fd, p, n);
  const int err = errno;
  if (rc < 0 && err == EPIPE && !was_pending) {
    const struct timespec zero = {0, 0};
    while (sigtimedwait(&pipe_set, nullptr, &zero) < 0 && errno == EINTR) {}
  }
  pthread_sigmask(SIG_SETMASK, &old, nullptr);
  errno = err;
  return rc;
}

int fd_send(void* user, const void* p, size_t n) {
  const vpin_wire* w = (const vpin_wire*)user;
  const uint8_t* b = (const uint8_t*)p;
  char why[160];
  size_t done = 0;
  while (done < n) {
    const int rc = wait_fd(w, w->wfd, POLLOUT, "waiting to send", done, n);
    if (rc) return rc;
    const size_t piece = w->w_is_socket ? n - done : (n - done < kPipePiece ? n - done : kPipePiece);
    const ssize_t k = w->w_is_socket ? send(w->wfd, b + done, piece, MSG_NOSIGNAL | MSG_DONTWAIT) : write_masked(w->wfd, b + done, piece);
    if (k > 0) { done += (size_t)k; continue; }
    if (k < 0 && (errno == EINTR || errno == EAGAIN || errno == EWOULDBLOCK)) continue;
    if (k < 0 && (errno == EPIPE || errno == ECONNRESET))
      snprintf(why, sizeof why, "vpin_wire: the peer closed the stream after %zu of %zu bytes were sent", done, n);
    else
      snprintf(why, sizeof why, "vpin_wire: write failed after %zu of %zu bytes: %s", done, n, k < 0 ? strerror(errno) : "nothing written");
    return fail(VPIN_ECOMM, why);
  }
  return VPIN_OK;
}

int fd_recv(void* user, void* p, size_t n) {
  const vpin_wire* w = (const vpin_wire*)user;
  uint8_t* b = (uint8_t*)p;
  char why[160];
  size_t done = 0;
  while (done < n) {
    const int rc = wait_fd(w, w->rfd, POLLIN, "waiting for the peer", done, n);
    if (rc) return rc;
    const ssize_t k = read(w->rfd, b + done, n - done);
    if (k > 0) { done += (size_t)k; continue; }
    if (k < 0 && (errno == EINTR || errno == EAGAIN || errno == EWOULDBLOCK)) continue;
    if (k == 0 || errno == ECONNRESET)
      snprintf(why, sizeof why, "vpin_wire: the peer closed the stream after %zu of %zu bytes", done, n);
    else
      snprintf(why, sizeof why, "vpin_wire: read failed after %zu of %zu bytes: %s", done, n, strerror(errno));
    return fail(VPIN_ECOMM, why);
  }
  return VPIN_OK;
}

}  // namespace

void add_ms(vpin_wire* w, size_t slot, Slot what, double ms) {
  if (slot >= ((size_t)1 << 16)) return;
  if (w->ms.size() <= slot) w->ms.resize(slot + 1, std::array<double, 4>{0.0, 0.0, 0.0, 0.0});
  w->ms[slot][what] += ms;
}

int send_all(vpin_wire* w, const void* p, size_t n) {
  if (!n) return VPIN_OK;
  set_error("");
  const int rc = w->io.send(w->io.user, p, n);
  if (rc) {
    if (!*vpin_last_error()) set_error("vpin_wire: the transport's send failed");
    return rc < 0 ? rc : VPIN_ECOMM;
  }
  w->stats[0] += n;
  return VPIN_OK;
}

int recv_all(vpin_wire* w, void* p, size_t n) {
  if (!n) return VPIN_OK;
  set_error("");
  const int rc = w->io.recv(w->io.user, p, n);
  if (rc) {
    if (!*vpin_last_error()) set_error("vpin_wire: the transport's recv failed");
    return rc < 0 ? rc : VPIN_ECOMM;
  }
  w->stats[1] += n;
  return VPIN_OK;
}

int send_frame(vpin_wire* w, const vpin_wire_header& h, const void* payload) {
  uint8_t head[VPIN_WIRE_HEADER_LEN];
  int rc = vpin_wire_header_encode(&h, head);
  if (rc) return rc;
  if (h.payload_len && !payload) return fail(VPIN_EINVAL, "vpin_wire_send: the frame has a payload and none is given");
  if ((rc = send_all(w, head, sizeof head))) return rc;
  if ((rc = send_all(w, payload, (size_t)h.payload_len))) return rc;
  w->stats[2]++;
  return VPIN_OK;
}

int recv_header(vpin_wire* w, vpin_wire_header* h) {
  uint8_t head[VPIN_WIRE_HEADER_LEN];
  int rc = recv_all(w, head, sizeof head);
  if (rc) return rc;
  if ((rc = vpin_wire_header_decode(head, h))) return rc;
  if (!h->payload_len) w->stats[3]++;  // the whole frame; one with a payload counts once that is in
  return VPIN_OK;
}

int recv_payload(vpin_wire* w, const vpin_wire_header& h, std::vector<uint8_t>* payload) {
  try {
    payload->resize((size_t)h.payload_len);  // at most 64 * VPIN_WIRE_MAX_CNT: decode has accepted the header
  } catch (const std::bad_alloc&) {
    return fail(VPIN_ENOMEM, "vpin_wire: no memory for the payload");
  }
  const int rc = recv_all(w, payload->data(), payload->size());
  if (!rc && h.payload_len) w->stats[3]++;
  return rc;
}

int discard_payload(vpin_wire* w, const vpin_wire_header& h) {
  uint8_t piece[4096];
  for (uint64_t left = h.payload_len; left;) {
    const size_t k = left < sizeof piece ? (size_t)left : sizeof piece;
    const int rc = recv_all(w, piece, k);
    if (rc) return rc;
    left -= k;
  }
  if (h.payload_len) w->stats[3]++;
  return VPIN_OK;
}

void send_error(vpin_wire* w, int code, const char* text) {
  char keep[VPIN_WIRE_MAX_TEXT + 1];
  snprintf(keep, sizeof keep, "%s", vpin_last_error());
  uint8_t payload[4 + VPIN_WIRE_MAX_TEXT];
  const size_t n = strnlen(text ? text : "", VPIN_WIRE_MAX_TEXT);
  const uint32_t c = (uint32_t)(int32_t)code;
  for (int i = 0; i < 4; i++) payload[i] = (uint8_t)(c >> (8 * i));
  memcpy(payload + 4, text ? text : "", n);
  vpin_wire_header h;
  memset(&h, 0, sizeof h);
  h.type = VPIN_WIRE_ERROR;
  h.payload_len = 4 + n;
  (void)send_frame(w, h, payload);
  set_error(keep);
}

int peer_error(vpin_wire* w, const vpin_wire_header& h, const char* who) {
  std::vector<uint8_t> p;
  const int rc = recv_payload(w, h, &p);
  if (rc) return rc;
  uint32_t c = 0;
  for (int i = 0; i < 4; i++) c |= (uint32_t)p[i] << (8 * i);
  char why[VPIN_WIRE_MAX_TEXT + 120];
  snprintf(why, sizeof why, "%s: the peer reported an error (%d): %.*s", who, (int)(int32_t)c, (int)(p.size() - 4), (const char*)p.data() + 4);
  return fail(VPIN_ECOMM, why);
}

}  // namespace vpin::wire

using namespace vpin::wire;

extern "C" {

int vpin_wire_create(const vpin_wire_io* io, vpin_wire** out) {
  if (out) *out = nullptr;
  if (!io || !io->send || !io->recv || !out) return fail(VPIN_EINVAL, "vpin_wire_create: null argument");
  vpin_wire* w = new (std::nothrow) vpin_wire();
  if (!w) return VPIN_ENOMEM;
  w->io = *io;
  *out = w;
  return VPIN_OK;
}

int vpin_wire_fd_create(int rfd, int wfd, int timeout_ms, vpin_wire** out) {
  if (out) *out = nullptr;
  if (!out) return fail(VPIN_EINVAL, "vpin_wire_fd_create: null argument");
  if (rfd < 0 || wfd < 0) return fail(VPIN_EINVAL, "vpin_wire_fd_create: a descriptor is negative");
  if (timeout_ms <= 0) return fail(VPIN_EINVAL, "vpin_wire_fd_create: timeout_ms must be positive");
  struct stat st;
  if (fstat(rfd, &st) || fstat(wfd, &st)) return fail(VPIN_EINVAL, "vpin_wire_fd_create: a descriptor is not open");
  vpin_wire* w = new (std::nothrow) vpin_wire();
  if (!w) return VPIN_ENOMEM;
  w->rfd = rfd; w->wfd = wfd; w->timeout_ms = timeout_ms;
  w->w_is_socket = S_ISSOCK(st.st_mode);  // st: the write side's
  w->io.send = fd_send; w->io.recv = fd_recv; w->io.user = w;
  *out = w;
  return VPIN_OK;
}

void vpin_wire_free(vpin_wire* w) { delete w; }

int vpin_wire_stats(const vpin_wire* w, uint64_t out[4]) {
  if (!w || !out) return fail(VPIN_EINVAL, "vpin_wire_stats: null argument");
  for (int i = 0; i < 4; i++) out[i] = w->stats[i];
  return VPIN_OK;
}

int vpin_wire_timings(const vpin_wire* w, size_t slot, double out[4]) {
  if (!w || !out) return fail(VPIN_EINVAL, "vpin_wire_timings: null argument");
  if (slot >= w->ms.size()) return fail(VPIN_EINVAL, "vpin_wire_timings: this wire has not seen that slot");
  for (int i = 0; i < 4; i++) out[i] = w->ms[slot][i];
  return VPIN_OK;
}

int vpin_wire_send(vpin_wire* w, const vpin_wire_header* h, const uint8_t* payload) {
  if (!w || !h) return fail(VPIN_EINVAL, "vpin_wire_send: null argument");
  return send_frame(w, *h, payload);
}

int vpin_wire_recv(vpin_wire* w, vpin_wire_header* h, uint8_t* payload, size_t cap) {
  if (!w || !h || (!payload && cap)) return fail(VPIN_EINVAL, "vpin_wire_recv: null argument");
  int rc = recv_header(w, h);
  if (rc) return rc;
  if (h->payload_len > cap) return fail(VPIN_EINVAL, "vpin_wire_recv: the frame's payload is longer than the buffer");
  if ((rc = recv_all(w, payload, (size_t)h->payload_len))) return rc;
  if (h->payload_len) w->stats[3]++;
  return VPIN_OK;
}

int vpin_wire_send_error(vpin_wire* w, int code, const char* text) {
  if (!w) return fail(VPIN_EINVAL, "vpin_wire_send_error: null argument");
  send_error(w, code, text);
  return VPIN_OK;
}

}  // extern "C"
