// Instance boxes from Cityscapes instance-id maps (*_gtFine_instanceIds.png): one pass over each map instead of the reference's
// per-id `inst_image == instance_id` + np.nonzero (data/datasets/cityscapes.py:501-540, which every rank repeats at start-up).
//
//   k_inst_accumulate  one workgroup per 2048-pixel tile of one map.  Each thread folds its 8 pixels into runs (same id, same row),
//                      the runs of the tile are merged in an LDS hash table (integer LDS atomics), then ONE set of global integer
//                      atomics per (workgroup, distinct id) updates the map's id table.  Integer min / max / add commute, so the table
//                      is bit-identical whatever order the workgroups arrive in.
//   k_inst_compact     one workgroup per map: an ordered scan of the id table (ascending id, = np.unique order) writes the records.
//
// Id table (workspace, zeroed by hipMemsetAsync): per map, per id in [24, 34000), five u32 fields all maximised or summed from 0:
//   W - xmin, H - ymin, xmax + 1, ymax + 1, pixel count.
#include "common.h"

#define INST_ID_LO 24          // ids below are stuff classes (cityscapes.py:503 filters inst_image >= 24 first)
#define INST_ID_HI 34000       // first id the Cityscapes label table cannot hold (label id = id // 1000 <= 33)
#define INST_NT (INST_ID_HI - INST_ID_LO)
#define INST_THREADS 256
#define INST_PPT 8                                  // pixels per thread: one 16-B load of u16 ids
#define INST_TILE (INST_THREADS * INST_PPT)         // pixels per workgroup
#define INST_HASH 4096                              // LDS hash slots: >= 2 x the distinct ids a tile can hold (load factor <= 0.5)
#define INST_EMPTY 0xffffffffu

static_assert(INST_HASH >= 2 * INST_TILE, "hash table must stay at most half full");

template <typename T>
__device__ __forceinline__ void inst_load(const T* p, long n_left, bool aligned, int (&v)[INST_PPT]) {
  if (n_left >= INST_PPT && aligned) {
    if constexpr (sizeof(T) == 2) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[2 * j] = (int)(q[j] & 0xffffu); v[2 * j + 1] = (int)(q[j] >> 16); }
    } else {
      const u32x4 q0 = reinterpret_cast<const u32x4*>(p)[0], q1 = reinterpret_cast<const u32x4*>(p)[1];
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = (int)q0[j]; v[4 + j] = (int)q1[j]; }
    }
  } else {
#pragma unroll
    for (int j = 0; j < INST_PPT; ++j) v[j] = j < n_left ? (sizeof(T) == 2 ? (int)(unsigned short)p[j] : (int)p[j]) : -1;
  }
}

template <typename T>
__global__ void __launch_bounds__(INST_THREADS) k_inst_accumulate(const T* __restrict__ maps, int H, int W,
                                                                   unsigned* __restrict__ table, unsigned* __restrict__ bad) {
  __shared__ unsigned hkey[INST_HASH];
  __shared__ unsigned short hent[INST_HASH];
  __shared__ unsigned ekey[INST_TILE];
  __shared__ unsigned eval_[5][INST_TILE];
  __shared__ unsigned nent;

  const int b = blockIdx.y, tid = threadIdx.x;
  const long HW = (long)H * W;
  const long p0 = (long)blockIdx.x * INST_TILE + (long)tid * INST_PPT;     // first pixel of this thread within map b
  for (int i = tid; i < INST_HASH; i += INST_THREADS) hkey[i] = INST_EMPTY;
  if (tid == 0) nent = 0;

  int v[INST_PPT];
  const T* src = maps + (long)b * HW + p0;
  inst_load<T>(src, p0 < HW ? HW - p0 : 0, ((size_t)src & 15) == 0, v);

  // runs of equal ids on one row, each identified by its first pixel j (static indices only: no scratch arrays)
  int xs[INST_PPT], ys[INST_PPT], len[INST_PPT];
  bool valid[INST_PPT], cont[INST_PPT];
  bool out_of_range = false;
  {
    int y = (int)(p0 / W), x = (int)(p0 - (long)y * W), prev = -1;
#pragma unroll
    for (int j = 0; j < INST_PPT; ++j) {
      xs[j] = x; ys[j] = y;
      out_of_range |= v[j] >= INST_ID_HI;
      valid[j] = v[j] >= INST_ID_LO && v[j] < INST_ID_HI;
      cont[j] = valid[j] && x > 0 && v[j] == prev;          // continues the previous pixel's run (same id, same row)
      prev = v[j];
      if (++x == W) { x = 0; ++y; }
    }
    int tail = 0;                                           // length of the run that continues from pixel j + 1
#pragma unroll
    for (int j = INST_PPT - 1; j >= 0; --j) {
      len[j] = valid[j] ? 1 + tail : 0;
      tail = cont[j] ? len[j] : 0;
    }
  }
  if (out_of_range) atomicOr(bad + b, 1u);
  __syncthreads();

  // phase 1: insert the runs' ids; the inserting thread claims and zeroes an entry
  int slot[INST_PPT];
#pragma unroll
  for (int r = 0; r < INST_PPT; ++r) {
    slot[r] = -1;
    if (valid[r] && !cont[r]) {
      const unsigned key = (unsigned)v[r];
      unsigned h = (key * 2654435761u) >> 20;                            // top 12 bits: INST_HASH = 4096
      while (true) {
        const unsigned prev = atomicCAS(&hkey[h], INST_EMPTY, key);
        if (prev == INST_EMPTY) {
          const unsigned e = atomicAdd(&nent, 1u);
          hent[h] = (unsigned short)e;
          ekey[e] = key;
#pragma unroll
          for (int f = 0; f < 5; ++f) eval_[f][e] = 0;
          break;
        }
        if (prev == key) break;
        h = (h + 1) & (INST_HASH - 1);
      }
      slot[r] = (int)h;
    }
  }
  __syncthreads();
  // phase 2: fold the runs into their entries (integer LDS atomics)
#pragma unroll
  for (int r = 0; r < INST_PPT; ++r) {
    if (slot[r] >= 0) {
      const unsigned e = hent[slot[r]];
      atomicMax(&eval_[0][e], (unsigned)(W - xs[r]));
      atomicMax(&eval_[1][e], (unsigned)(H - ys[r]));
      atomicMax(&eval_[2][e], (unsigned)(xs[r] + len[r]));
      atomicMax(&eval_[3][e], (unsigned)(ys[r] + 1));
      atomicAdd(&eval_[4][e], (unsigned)len[r]);
    }
  }
  __syncthreads();
  // phase 3: one set of global atomics per (workgroup, id)
  const unsigned n = nent;
  unsigned* tb = table + (long)b * 5 * INST_NT;
  for (unsigned e = tid; e < n; e += INST_THREADS) {
    const unsigned i = ekey[e] - INST_ID_LO;
    atomicMax(tb + 0 * INST_NT + i, eval_[0][e]);
    atomicMax(tb + 1 * INST_NT + i, eval_[1][e]);
    atomicMax(tb + 2 * INST_NT + i, eval_[2][e]);
    atomicMax(tb + 3 * INST_NT + i, eval_[3][e]);
    atomicAdd(tb + 4 * INST_NT + i, eval_[4][e]);
  }
}

#define INST_CT 1024
__global__ void __launch_bounds__(INST_CT) k_inst_compact(const unsigned* __restrict__ table, const unsigned* __restrict__ bad, int H,
                                                          int W, int* __restrict__ rec, int max_rec, int* __restrict__ counts) {
  __shared__ int wsum[INST_CT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned* tb = table + (long)b * 5 * INST_NT;
  int* out = rec + (long)b * max_rec * 6;
  int base = 0;
  for (int i0 = 0; i0 < INST_NT; i0 += INST_CT) {
    const int i = i0 + tid;
    const bool hit = i < INST_NT && tb[4 * INST_NT + i] != 0;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < INST_CT / 64; ++w) {
      before += w < wave ? wsum[w] : 0;
      total += wsum[w];
    }
    if (hit) {
      const int o = base + before + __popcll(m & ((1ull << lane) - 1));
      if (o < max_rec) {
        int* r = out + (long)o * 6;
        r[0] = i + INST_ID_LO;
        r[1] = W - (int)tb[0 * INST_NT + i];
        r[2] = H - (int)tb[1 * INST_NT + i];
        r[3] = (int)tb[2 * INST_NT + i] - 1;
        r[4] = (int)tb[3 * INST_NT + i] - 1;
        r[5] = (int)tb[4 * INST_NT + i];
      }
    }
    base += total;
    __syncthreads();                                   // wsum is rewritten by the next round
  }
  if (tid == 0) counts[b] = bad[b] ? -1 : (base < max_rec ? base : max_rec);
}

extern "C" int cddmsl_instance_boxes(const void* maps, int B, int H, int W, int dtype, int* records, int max_records, int* counts,
                                     void* ws, size_t* ws_bytes, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (dtype != 0 && dtype != 1) || !ws_bytes || B > 65535)
    return CDDMSL_ERR_ARG;
  const size_t table_bytes = (size_t)B * 5 * INST_NT * sizeof(unsigned);
  const size_t need = table_bytes + (size_t)B * sizeof(unsigned);
  if (!ws) { *ws_bytes = need; return CDDMSL_OK; }
  if (*ws_bytes < need || !maps || !records || !counts || max_records < 0) return CDDMSL_ERR_ARG;
  // every distinct id of a map gets a record: the buffer must hold min(ids in range, pixels) of them
  const long HW = (long)H * W;
  if ((long)max_records < (HW < INST_NT ? HW : (long)INST_NT)) return CDDMSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned* table = (unsigned*)ws;
  unsigned* bad = (unsigned*)((char*)ws + table_bytes);
  if (hipMemsetAsync(ws, 0, need, st) != hipSuccess) return CDDMSL_ERR_LAUNCH;
  const long tiles = (HW + INST_TILE - 1) / INST_TILE;
  if (tiles > 0x7fffffffL) return CDDMSL_ERR_ARG;
  const dim3 grid((unsigned)tiles, (unsigned)B);
  if (dtype == 0)
    k_inst_accumulate<unsigned short><<<grid, dim3(INST_THREADS), 0, st>>>((const unsigned short*)maps, H, W, table, bad);
  else
    k_inst_accumulate<int><<<grid, dim3(INST_THREADS), 0, st>>>((const int*)maps, H, W, table, bad);
  if (hipGetLastError() != hipSuccess) return CDDMSL_ERR_LAUNCH;
  k_inst_compact<<<dim3(B), dim3(INST_CT), 0, st>>>(table, bad, H, W, records, max_records, counts);
  return hipGetLastError() == hipSuccess ? CDDMSL_OK : CDDMSL_ERR_LAUNCH;
}
