// Host-only reader of the binary vocabulary file and the checks a tree must pass before it goes to the device.  No HIP in here:
// tests/cpp/vocab_file_check.cpp builds this header alone under the host sanitizers.
// Layout (TemplatedVocabulary::loadFromBinaryFile, /root/reference/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1343-1384):
//   u32 nb_nodes, u32 size_node, i32 k, i32 L, i32 scoring, i32 weighting, then nb_nodes records of size_node = 41 bytes:
//   i32 parent, 32 B descriptor, f32 weight, u8 leaf.  Record i is node i + 1; the root is node 0.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#define PS_VOCAB_RECORD_BYTES 41
#define PS_VOCAB_HEADER_BYTES 24
#define PS_VOCAB_MAX_K 20
#define PS_VOCAB_MAX_L 10

struct PsVocabFile {
  int32_t k = 0, L = 0, scoring = 0, weighting = 0;
  std::vector<int32_t> parent;
  std::vector<uint8_t> desc;      // [n][32]
  std::vector<float> weight;
  std::vector<uint8_t> is_leaf;
  int nnodes() const { return (int)parent.size(); }
};

// Reads `path`.  Empty string on success, else what is wrong with the file.
inline std::string ps_vocab_file_read(const char* path, PsVocabFile& out) {
  out = PsVocabFile();
  if (!path) return "null path";
  FILE* f = fopen(path, "rb");
  if (!f) return std::string("cannot open ") + path;
  std::string err;
  do {
    if (fseek(f, 0, SEEK_END) != 0) { err = "cannot seek"; break; }
    const long len = ftell(f);
    if (len < 0 || fseek(f, 0, SEEK_SET) != 0) { err = "cannot seek"; break; }
    uint8_t head[PS_VOCAB_HEADER_BYTES];
    if (len < PS_VOCAB_HEADER_BYTES || fread(head, 1, PS_VOCAB_HEADER_BYTES, f) != PS_VOCAB_HEADER_BYTES) { err = "truncated header"; break; }
    uint32_t nb = 0, size_node = 0;
    memcpy(&nb, head, 4); memcpy(&size_node, head + 4, 4);
    memcpy(&out.k, head + 8, 4); memcpy(&out.L, head + 12, 4); memcpy(&out.scoring, head + 16, 4); memcpy(&out.weighting, head + 20, 4);
    if (size_node != PS_VOCAB_RECORD_BYTES) { err = "size_node is " + std::to_string(size_node) + ", not 41"; break; }
    if (nb > 0x7FFFFFF0u) { err = "nb_nodes out of range"; break; }
    const unsigned long long want = (unsigned long long)PS_VOCAB_HEADER_BYTES + (unsigned long long)nb * PS_VOCAB_RECORD_BYTES;
    if ((unsigned long long)len < want) { err = "truncated: " + std::to_string(nb) + " records need " + std::to_string(want) + " bytes, the file has " + std::to_string(len); break; }
    if ((unsigned long long)len > want) { err = "the file has " + std::to_string(len) + " bytes, " + std::to_string(nb) + " records end at " + std::to_string(want); break; }
    out.parent.resize(nb); out.desc.resize((size_t)nb * 32); out.weight.resize(nb); out.is_leaf.resize(nb);
    std::vector<uint8_t> buf((size_t)4096 * PS_VOCAB_RECORD_BYTES);
    for (size_t i0 = 0; i0 < nb && err.empty(); i0 += 4096) {
      const size_t cnt = nb - i0 < 4096 ? nb - i0 : 4096;
      if (fread(buf.data(), PS_VOCAB_RECORD_BYTES, cnt, f) != cnt) { err = "short read"; break; }
      for (size_t j = 0; j < cnt; j++) {
        const uint8_t* r = buf.data() + j * PS_VOCAB_RECORD_BYTES;
        memcpy(&out.parent[i0 + j], r, 4);
        memcpy(&out.desc[(i0 + j) * 32], r + 4, 32);
        memcpy(&out.weight[i0 + j], r + 36, 4);
        out.is_leaf[i0 + j] = r[40] ? 1 : 0;
      }
    }
  } while (false);
  fclose(f);
  if (!err.empty()) out = PsVocabFile();
  return err;
}

// The conditions under which the reference's loader and descent stay inside defined behaviour, plus the parameter ranges the
// library accepts.  Empty string when the tree is usable.
inline std::string ps_vocab_check(int k, int L, int scoring, int weighting, int nnodes, const int32_t* parent, const uint8_t* is_leaf) {
  if (k < 1 || k > PS_VOCAB_MAX_K) return "k out of range (1..20)";
  if (L < 1 || L > PS_VOCAB_MAX_L) return "L out of range (1..10)";
  if (scoring != 0) return "only L1_NORM scoring is supported";
  if (weighting < 0 || weighting > 3) return "unknown weighting";
  if (nnodes < 1 || nnodes > 0x7FFFFFF0 || !parent || !is_leaf) return "no nodes";
  std::vector<uint8_t> has_child((size_t)nnodes + 1, 0);
  for (int i = 0; i < nnodes; i++) {
    const int32_t p = parent[i];
    if (p < 0 || p > i) return "record " + std::to_string(i) + ": parent " + std::to_string(p) + " does not precede node " + std::to_string(i + 1);
    if (p > 0 && is_leaf[p - 1]) return "record " + std::to_string(i) + ": parent " + std::to_string(p) + " is a leaf";
    has_child[p] = 1;
  }
  if (!has_child[0]) return "the root has no children";
  for (int i = 0; i < nnodes; i++)
    if (!is_leaf[i] && !has_child[(size_t)i + 1]) return "node " + std::to_string(i + 1) + " is an inner node with no children";
  return std::string();
}
