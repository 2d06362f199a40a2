// The matcher handle as the host side of the library sees it: match_host.hip owns it, bow_host.hip runs its calls on it.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdint.h>

struct ps_matcher {
  std::mutex mu;              // calls on one handle are serialised (a handle may be shared by threads)
  int device = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_buf = nullptr;   // one growable device arena
  size_t d_bytes = 0;
  uint8_t* h_buf = nullptr;   // pinned staging of the same size
  size_t h_bytes = 0;
  uint8_t* d_wide = nullptr;  // second arena, only for the wide re-run of search problems whose windows overflowed the candidate store
  size_t d_wide_bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the kernels of the last brute-force / projection / triangulation / bag-of-words call (ps_matcher_last_kernel_ms)
  float last_kernel_ms = 0;
};

// grows both arenas to at least `need` bytes (contents are lost); PS_OK or PS_ERR_HIP
int psm_ensure(ps_matcher* m, size_t need);
