// Kernels of the frame handle (ps_frame, include/pointslot_hip.h).
//   frame_publish : a stereo Frame's search-relevant state from keypoints (cv::KeyPoint layout), mvuRight and mDescriptors to the
//                   SoA the windowed matchers read, plus Frame::AssignFeaturesToGrid / PosInGrid as CSR
//                   (/root/reference/src/Frame.cc:1636-1656, 2027-2037).  One workgroup per frame.
//   frame_stage   : the train sides of the frame-backed problems of one search call, from their slabs into the matcher's arena.
// Compiled with -ffp-contract=off: PosInGrid is evaluated as written, round((x - mnMinX) * mfGridElementWidthInv) in float.
#include <hip/hip_runtime.h>
#include "frame_plan.h"

namespace {

// Frame::PosInGrid; -1 for a keypoint outside the grid (it is in no cell's list).  The range test is made on the rounded float,
// which is the same test for every value an int holds and is defined for the others.
__device__ inline int frame_cell(float x, float y, float min_x, float min_y, float gw_inv, float gh_inv) {
  const float fx = roundf((x - min_x) * gw_inv), fy = roundf((y - min_y) * gh_inv);
  if (!(fx >= 0.f && fx < (float)PS_GRID_COLS && fy >= 0.f && fy < (float)PS_GRID_ROWS)) return -1;
  return (int)fx * PS_GRID_ROWS + (int)fy;
}

}  // namespace

// The CSR lists must be in ascending keypoint index whatever the scheduling, at a cost that does not depend on how the keypoints are
// spread over the cells.  Each of the 4 waves owns a contiguous quarter of the keypoints and a private histogram in LDS:
//   pass 1  SoA conversion; every wave counts its keypoints per cell (LDS adds into its own histogram: a count has no order);
//   scan    over cells, and inside a cell over the waves: cell_off, and for every (wave, cell) the slot of the wave's first keypoint;
//   pass 2  a wave walks its quarter 64 keypoints at a time in index order.  A lane's rank among the lanes of the same cell comes
//           from 13 ballots (one per bit of the cell id, one for "in the grid"); slot = the wave's cursor of the cell + rank, and the
//           last lane of each cell advances the cursor.  No atomics, no sort, the same work for one crowded cell as for 3072.
extern "C" __global__ __launch_bounds__(PS_FRAME_PUB_THREADS) void frame_publish(const FramePubBatch B) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* wcnt = reinterpret_cast<int32_t*>(smem);                    // [PS_FRAME_PUB_WAVES][PS_FRAME_NCELL]
  int32_t* red = wcnt + PS_FRAME_PUB_WAVES * PS_FRAME_NCELL;          // [PS_FRAME_PUB_THREADS] scan scratch, [.. + 1] total
  const FramePubJob& J = B.job[blockIdx.x];
  const FrameSlab S = J.dst;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int n = J.n, mismatch = 0;
  if (J.count) {
    const int have = *J.count;
    mismatch = have != n;
    n = n < have ? n : have;
  }
  n = n < 0 ? 0 : (n > J.capacity ? J.capacity : n);
  // what an earlier, larger publish (or a count larger than the device's) left behind is cleared up to here
  int old_n = J.prev_n > J.n ? J.prev_n : J.n;
  old_n = old_n > J.capacity ? J.capacity : old_n;
  const float min_x = J.min_x, min_y = J.min_y, gw_inv = J.gw_inv, gh_inv = J.gh_inv;

  for (int i = tid; i < PS_FRAME_PUB_WAVES * PS_FRAME_NCELL; i += PS_FRAME_PUB_THREADS) wcnt[i] = 0;
  __syncthreads();

  const int per = ((n + PS_FRAME_PUB_WAVES - 1) / PS_FRAME_PUB_WAVES + 63) & ~63;   // keypoints per wave, whole chunks
  const int b = w * per < n ? w * per : n, e = b + per < n ? b + per : n;
  int32_t* mine = wcnt + w * PS_FRAME_NCELL;
  for (int i = b + lane; i < e; i += 64) {
    const ps_keypoint k = J.kps[i];
    S.x[i] = k.x; S.y[i] = k.y; S.octave[i] = k.octave; S.angle[i] = k.angle;
    S.u_right[i] = J.u_right ? J.u_right[i] : -1.f;
    const int c = frame_cell(k.x, k.y, min_x, min_y, gw_inv, gh_inv);
    if (c >= 0) atomicAdd(&mine[c], 1);
  }
  for (int i = n + tid; i < old_n; i += PS_FRAME_PUB_THREADS) { S.x[i] = 0.f; S.y[i] = 0.f; S.octave[i] = 0; S.angle[i] = 0.f; S.u_right[i] = 0.f; }
  {
    // descriptors: two 16-byte pieces per keypoint, consecutive lanes on consecutive pieces
    const uint4* sd = reinterpret_cast<const uint4*>(J.desc);
    uint4* dd = reinterpret_cast<uint4*>(S.desc);
    for (int k = tid; k < 2 * n; k += PS_FRAME_PUB_THREADS) dd[k] = sd[k];
    for (int k = 2 * n + tid; k < 2 * old_n; k += PS_FRAME_PUB_THREADS) dd[k] = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();

  // ---- exclusive scan: 12 cells per thread, inside a cell the waves in order ----
  {
    static_assert(PS_FRAME_NCELL % PS_FRAME_PUB_THREADS == 0, "the cell scan takes a whole number of cells per thread");
    const int per_t = PS_FRAME_NCELL / PS_FRAME_PUB_THREADS;
    int sum = 0;
    for (int k = 0; k < per_t; k++)
      for (int v = 0; v < PS_FRAME_PUB_WAVES; v++) sum += wcnt[v * PS_FRAME_NCELL + tid * per_t + k];
    red[tid] = sum;
    __syncthreads();
    for (int d = 1; d < PS_FRAME_PUB_THREADS; d <<= 1) {
      const int add = tid >= d ? red[tid - d] : 0;
      __syncthreads();
      red[tid] += add;
      __syncthreads();
    }
    int off = red[tid] - sum;
    if (tid == PS_FRAME_PUB_THREADS - 1) { red[PS_FRAME_PUB_THREADS] = red[tid]; S.cell_off[PS_FRAME_NCELL] = red[tid]; }
    for (int k = 0; k < per_t; k++) {
      const int c = tid * per_t + k;
      S.cell_off[c] = off;
      for (int v = 0; v < PS_FRAME_PUB_WAVES; v++) {
        const int t = wcnt[v * PS_FRAME_NCELL + c];
        wcnt[v * PS_FRAME_NCELL + c] = off;
        off += t;
      }
    }
  }
  __syncthreads();

  // ---- fill: every wave its own quarter, in index order ----
  const unsigned long long below = (1ull << lane) - 1ull, above = ~((2ull << lane) - 1ull);
  for (int base = b; base < e; base += 64) {       // (uniform trip count: all 64 lanes take part in the ballots)
    const int i = base + lane;
    int c = -1;
    if (i < e) {
      const ps_keypoint k = J.kps[i];
      c = frame_cell(k.x, k.y, min_x, min_y, gw_inv, gh_inv);
    }
    unsigned long long same = __ballot(c >= 0);
    for (int bit = 0; bit < 12; bit++) {           // 3072 cells: 12 bits
      const int mine_bit = (c >> bit) & 1;
      const unsigned long long set = __ballot(mine_bit);
      same &= mine_bit ? set : ~set;
    }
    if (c >= 0) {
      const int slot = mine[c] + __popcll(same & below);
      S.cell_idx[slot] = i;
      if ((same & above) == 0ull) mine[c] = slot + 1;   // one lane per distinct cell of the chunk
    }
    __builtin_amdgcn_wave_barrier();
  }
  const int total = red[PS_FRAME_PUB_THREADS];
  for (int i = total + tid; i < old_n; i += PS_FRAME_PUB_THREADS) S.cell_idx[i] = 0;   // keypoints outside the grid leave a tail
  if (tid == 0) { S.hdr->n = n; S.hdr->mismatch = mismatch; S.hdr->pad[0] = 0; S.hdr->pad[1] = 0; }
}

extern "C" __global__ __launch_bounds__(256) void frame_stage(const FrameStageJob* __restrict__ jobs, const FrameStageDst D) {
  const FrameStageJob J = jobs[blockIdx.y];
  const FrameSlab S = J.src;
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  const int n = J.nt;
  const size_t t0 = (size_t)J.t_off;
  for (int i = tid; i < n; i += nth) {
    D.tx[t0 + i] = S.x[i]; D.ty[t0 + i] = S.y[i]; D.toct[t0 + i] = S.octave[i]; D.tur[t0 + i] = S.u_right[i];
    if (D.cell_idx) D.cell_idx[t0 + i] = S.cell_idx[i];
    if (D.tang) D.tang[t0 + i] = S.angle[i];
  }
  {
    const uint4* sd = reinterpret_cast<const uint4*>(S.desc);
    uint4* dd = reinterpret_cast<uint4*>(D.tdesc + t0 * 32);
    for (int k = tid; k < 2 * n; k += nth) dd[k] = sd[k];
  }
  if (D.cell_off)
    for (int i = tid; i <= PS_FRAME_NCELL; i += nth) D.cell_off[(size_t)J.grid_off + i] = S.cell_off[i];
  if (tid == 0) D.status[J.prob] = (S.hdr->n != n || S.hdr->mismatch) ? 1 : 0;
}

extern "C" {
void psk_frame_publish_launch(const FramePubBatch* batch, int nframes, hipStream_t st) {
  const size_t lds = ((size_t)PS_FRAME_PUB_WAVES * PS_FRAME_NCELL + PS_FRAME_PUB_THREADS + 4) * sizeof(int32_t);
  hipLaunchKernelGGL(frame_publish, dim3(nframes), dim3(PS_FRAME_PUB_THREADS), lds, st, *batch);
}
void psk_frame_stage_launch(const FrameStageJob* d_jobs, int njobs, const FrameStageDst* dst, hipStream_t st) {
  hipLaunchKernelGGL(frame_stage, dim3(8, njobs), dim3(256), 0, st, d_jobs, *dst);
}
}
