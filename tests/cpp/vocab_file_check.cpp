// Stand-alone check of the host-only vocabulary file reader (pointslot_amd/csrc/vocab_file.h), built by tests/test_bow_cpu.py
// with -fsanitize=address,undefined.  Arguments: a file written by pointslot_amd.bow.save_binary with what it holds (records,
// leaves, sum of weights, sum of parents, sum of descriptor bytes), then seven damaged files that must be refused with a
// message: truncated, short header, size_node 40, a record count above and one below the file's length, a parent that does not
// precede its child, a negative parent.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "vocab_file.h"

static int checks = 0, failed = 0;
static void expect(bool ok, const char* what, const std::string& detail = std::string()) {
  checks++;
  if (!ok) { failed++; printf("FAILED %s %s\n", what, detail.c_str()); }
  else printf("passed %s %s\n", what, detail.c_str());
}

int main(int argc, char** argv) {
  if (argc != 14) { printf("usage: good n leaves wsum psum dsum truncated short_head size40 more fewer forward negative\n"); return 2; }
  PsVocabFile F;
  std::string err = ps_vocab_file_read(argv[1], F);
  bool ok = err.empty() && F.nnodes() == atoi(argv[2]);
  if (ok) {
    long long leaves = 0, psum = 0, dsum = 0;
    double wsum = 0;
    for (int i = 0; i < F.nnodes(); i++) { leaves += F.is_leaf[i]; psum += F.parent[i]; wsum += (double)F.weight[i]; }
    for (uint8_t b : F.desc) dsum += b;
    ok = leaves == atoll(argv[3]) && std::fabs(wsum - atof(argv[4])) <= 1e-9 * std::fabs(wsum) && psum == atoll(argv[5]) && dsum == atoll(argv[6]);
    ok = ok && ps_vocab_check(F.k, F.L, F.scoring, F.weighting, F.nnodes(), F.parent.data(), F.is_leaf.data()).empty();
  }
  expect(ok, "round trip", err);
  const char* refused[] = {"truncated", "short header", "size_node 40", "more records than bytes", "fewer records than bytes"};
  for (int i = 0; i < 5; i++) {
    err = ps_vocab_file_read(argv[7 + i], F);
    expect(!err.empty() && F.nnodes() == 0, refused[i], err);
  }
  const char* tree[] = {"parent does not precede", "negative parent"};
  for (int i = 0; i < 2; i++) {
    err = ps_vocab_file_read(argv[12 + i], F);
    std::string why = err.empty() ? ps_vocab_check(F.k, F.L, F.scoring, F.weighting, F.nnodes(), F.parent.data(), F.is_leaf.data()) : "unreadable: " + err;
    expect(err.empty() && !why.empty(), tree[i], why);
  }
  if (failed) { printf("%d of %d checks failed\n", failed, checks); return 1; }
  printf("ok %d checks\n", checks);
  return 0;
}
