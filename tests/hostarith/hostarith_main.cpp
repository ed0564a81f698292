// hostarith_main.cpp -- the harness of hostarith.cpp as a program of its own, so that the host arithmetic can run under the
// address and undefined-behaviour sanitizers in a child process (sanitized code is never loaded into python).
//
//   hostarith_main VECTORS
//
// VECTORS is what tests/host_vectors.py:write_vector_file writes: blocks of "<function> <n>" followed by n * IW words in
// hexadecimal.  For every block the program prints "<function> <n>" and n lines of OW hexadecimal words.  Exit status 0 when
// every block ran, 2 on a malformed file or an unknown function.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct hv_entry { const char* name; int iw, ow; int (*fn)(const uint64_t*, uint64_t*, int); };
extern "C" int hv_table(const hv_entry** out);

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s VECTORS\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  const hv_entry* tab;
  const int nt = hv_table(&tab);
  char name[64];
  int n, status = 0;
  while (fscanf(f, "%63s %d", name, &n) == 2) {
    const hv_entry* e = nullptr;
    for (int i = 0; i < nt; i++)
      if (!strcmp(tab[i].name, name)) e = &tab[i];
    if (!e || n < 0) { fprintf(stderr, "unknown function or bad count: %s %d\n", name, n); status = 2; break; }
    std::vector<uint64_t> in((size_t)n * e->iw), out((size_t)n * e->ow, 0xa5a5a5a5a5a5a5a5ULL);
    bool ok = true;
    for (auto& w : in) ok = ok && fscanf(f, "%" SCNx64, &w) == 1;
    if (!ok) { fprintf(stderr, "%s: short block\n", name); status = 2; break; }
    if (e->fn(in.data(), out.data(), n) != 0) { fprintf(stderr, "%s failed\n", name); status = 2; break; }
    printf("%s %d\n", name, n);
    for (int i = 0; i < n; i++) {
      for (int k = 0; k < e->ow; k++) printf("%s%" PRIx64, k ? " " : "", out[(size_t)i * e->ow + k]);
      printf("\n");
    }
  }
  fclose(f);
  return status;
}
