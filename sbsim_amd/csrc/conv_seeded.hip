// conv_seeded.hip -- the reference's seeded convection shuffle on the device, one Mersenne Twister per building
// (sb_convection_attach_seeded): every building of a batch stands for a reference process that called
// random.seed(seed_b) once, and k_convect_seeded consumes that stream draw for draw (conv_seeded.h), so a building's grid
// after every step is the finite-difference grid with the reference's own permutation applied, bit for bit.  The
// counter-based shuffle (generators.hip: k_convect, k_convect_all) stays the fast default; this mode shares its tables
// (ConvCell, partner, by_rank).
#include "sb_host.h"

#include "conv_seeded.h"

using namespace sb;

namespace {

constexpr int kSeededThreads = 64;         // one wavefront per building at a time
constexpr int kSeededMaxWorkgroups = 4096; // the grid's cap (16 per CU of an MI355X); buildings beyond it: grid stride
constexpr int kSeededMaxRoom = 2047;       // as k_convect: a cell's rank and a pick share one 32-bit record

struct SeededArgs {
  double *temp;
  size_t stride;                 // doubles per building
  const int *zone_off, *by_rank; // by_rank[zone_off[z] + r]: index (in the zone's ConvCell list) of the cell with raster rank r
  const ConvCell *cells;         // .pad: the cell's rank, .mask: its valid offsets, .sidx: its index in the state
  const unsigned short *partner; // [cells][pw]: a cell's candidates in window raster order, as list indices
  uint32_t *rng;                 // [B][625] the buildings' generators
  int pw, B, Z, max_room, whole_room;
  double p;
};

// What the draws depend on is the data: where cell i starts reading depends on how many tries every earlier cell
// needed.  So a building is ONE serial chain, and the kernel keeps each link to LDS and scalar traffic: the block of
// 624 words sits in LDS already tempered, every lane runs the consumer on the same values (LDS broadcasts, words taken
// into scalar registers: the control flow is the wavefront's, not the lanes'), and nothing in the chain reads global
// memory.  Around the chain the lanes work in parallel: they load a room's values and candidate counts, resolve the
// recorded picks to cells through the partner table, regenerate the block, and scatter the room back.
//   LDS (dynamic, 13 * max_room rounded up to 8, + 4992 bytes): val [max_room] double | rec [max_room] uint32 | mt [624] |
//   out [624] (tempered) | cnt [max_room] uint8.  Everything is indexed by a cell's RANK in its room (the caller's raster
//   order), below max_room; mt / out by an index the source keeps below 624.
struct LdsSource {
  uint32_t *mt, *out;
  uint32_t idx; // < 624, or 624: regenerate first (wavefront-uniform)
  __device__ inline void temper_all() {
    for (int k = threadIdx.x; k < sbconv::kMtN; k += kSeededThreads) out[k] = sbconv::mt_temper(mt[k]);
    __syncthreads();
  }
  // all lanes, 64 words at a time in increasing order: a run's reads come before its writes (conv_seeded.h, mt_twist)
  __device__ inline void regenerate() {
    for (int base = 0; base < sbconv::kMtN; base += kSeededThreads) {
      const int k = base + (int)threadIdx.x;
      uint32_t v = 0;
      if (k < sbconv::kMtN) {
        const int k1 = k + 1 < sbconv::kMtN ? k + 1 : 0;
        const int km = k + sbconv::kMtM < sbconv::kMtN ? k + sbconv::kMtM : k + sbconv::kMtM - sbconv::kMtN;
        v = sbconv::mt_twist(mt[k], mt[k1], mt[km]);
      }
      __syncthreads();
      if (k < sbconv::kMtN) { mt[k] = v; out[k] = sbconv::mt_temper(v); }
      __syncthreads();
    }
    idx = 0;
  }
  __device__ inline uint32_t next() {
    if (idx >= (uint32_t)sbconv::kMtN) regenerate();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)out[idx++]);
  }
};

__global__ void __launch_bounds__(kSeededThreads) k_convect_seeded(SeededArgs o) {
  extern __shared__ __attribute__((aligned(16))) double seeded_lds[];
  const int M = o.max_room;
  double *val = seeded_lds;              // [M]
  uint32_t *rec = (uint32_t *)(val + M); // [M]
  LdsSource src;
  src.mt = rec + M;                      // [624]
  src.out = src.mt + sbconv::kMtN;       // [624]
  uint8_t *cnt = (uint8_t *)(src.out + sbconv::kMtN); // [M]
  const int lane = threadIdx.x;
  for (int b = blockIdx.x; b < o.B; b += gridDim.x) {
    double *st = o.temp + (size_t)b * o.stride;
    uint32_t *row = o.rng + (size_t)b * sbconv::kRngWords;
    for (int k = lane; k < sbconv::kMtN; k += kSeededThreads) src.mt[k] = row[k];
    const uint32_t stored = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[sbconv::kMtN]);
    src.idx = stored > (uint32_t)sbconv::kMtN ? (uint32_t)sbconv::kMtN : stored; // whatever sb_convection_rng_set was given
    __syncthreads();
    src.temper_all();
    for (int z = 0; z < o.Z; ++z) {
      const int c0 = o.zone_off[z];
      int n = o.zone_off[z + 1] - c0;
      n = n < 0 ? 0 : n > M ? M : n; // (the host built both from the same lists)
      if (o.whole_room) {
        for (int r = lane; r < n; r += kSeededThreads) {
          val[r] = st[o.cells[c0 + o.by_rank[c0 + r]].sidx];
          rec[r] = (uint32_t)r;
        }
        __syncthreads();
        sbconv::shuffle(src, rec, n);
        __syncthreads();
        for (int r = lane; r < n; r += kSeededThreads) // the value of cell r goes to cell order[r]
          st[o.cells[c0 + o.by_rank[c0 + (int)rec[r]]].sidx] = val[r];
        __syncthreads();
        continue;
      }
      for (int r = lane; r < n; r += kSeededThreads) {
        const ConvCell c = o.cells[c0 + o.by_rank[c0 + r]];
        val[r] = st[c.sidx];
        const int cands = __popcll(c.mask);
        cnt[r] = (uint8_t)(cands < 1 ? 1 : cands > o.pw ? o.pw : cands); // 1 .. pw: a pick stays inside the cell's partner row
      }
      __syncthreads();
      // the chain: (cell, pick) pairs only
      const int m = __builtin_amdgcn_readfirstlane(sbconv::room_draws(src, n, o.p, cnt, rec));
      __syncthreads();
      // the pick-th candidate of each moving cell, as a rank
      for (int k = lane; k < m; k += kSeededThreads) {
        const uint32_t w = rec[k], r = w >> 16, pick = w & 0xffffu;
        const int i = o.by_rank[c0 + (int)r];
        int j = (int)o.partner[(size_t)(c0 + i) * (size_t)o.pw + (size_t)pick];
        j = j < n ? j : i;
        int rj = o.cells[c0 + j].pad;
        rj = rj >= 0 && rj < n ? rj : (int)r;
        rec[k] = (r << 16) | (uint32_t)rj;
      }
      __syncthreads();
      sbconv::shuffle(src, rec, m);
      __syncthreads();
      sbconv::room_swaps(rec, m, val);
      __syncthreads();
      for (int r = lane; r < n; r += kSeededThreads) st[o.cells[c0 + o.by_rank[c0 + r]].sidx] = val[r];
      __syncthreads();
    }
    for (int k = lane; k < sbconv::kMtN; k += kSeededThreads) row[k] = src.mt[k];
    if (lane == 0) row[sbconv::kMtN] = src.idx;
    __syncthreads();
  }
}

size_t seeded_lds_bytes(int max_room) {
  return ((size_t)max_room * (8 + 4 + 1) + 7) / 8 * 8 + (size_t)2 * sbconv::kMtN * sizeof(uint32_t);
}

} // namespace

extern "C" {

int sb_convection_attach_seeded(sb_handle *h, double p, int32_t distance, const uint64_t *seeds_host, int32_t transposed) {
  const std::string who = "sb_convection_attach_seeded";
  if (!h) return fail(SB_ERR_INVALID, who + ": null handle");
  const std::string host_mode = " (the host mode replays those: host_convection.SeededHostConvection, HipSimulatorBuilding("
                                "reproducible_convection=True))";
  if (h->kernel == SB_KERNEL_JACOBI) return fail(SB_ERR_UNSUPPORTED, who + ": not implemented for the Jacobi solver" + host_mode);
  if (!(p >= 0.0 && p <= 1.0)) return fail(SB_ERR_INVALID, who + ": p must be in [0, 1]");
  if (p == 0.0 || distance == 0) { h->conv_attached = false; h->conv_seeded = false; return SB_OK; } // :70-71
  if (!seeds_host) return fail(SB_ERR_INVALID, who + ": null seeds");
  const bool whole_room = distance == -1 && p == 1.0;
  if (!whole_room) {
    if (distance < -1 || distance > 1000)
      return fail(SB_ERR_UNSUPPORTED, who + ": distance must be 1..19, or -1 with p = 1 (the whole-room shuffle)");
    // the windows sb_convection_attach builds partner tables for: at most 64 offsets, distance 1..19
    const int dist = distance == -1 ? 1000 : distance, reach = std::min(dist, 32);
    int n_off = 0;
    for (int dx = -reach; dx < reach; ++dx)
      for (int dy = -reach; dy < reach; ++dy) n_off += dx * dx + dy * dy <= dist;
    if (n_off > 64)
      return fail(SB_ERR_UNSUPPORTED, who + ": a window of more than 64 offsets (distance >= 20, or -1 with p < 1) is not "
                                            "replayed on the device" + host_mode);
  }
  for (int z = 0; z < h->d.Z; ++z)
    if (h->h_zone_off[z + 1] - h->h_zone_off[z] > kSeededMaxRoom)
      return fail(SB_ERR_UNSUPPORTED, who + ": a room has more than 2047 cells" + host_mode);
  // the generators, seeded as random.seed(seed_b) seeds: built before anything changes
  const size_t B = (size_t)h->d.B;
  std::vector<uint32_t> table(B * sbconv::kRngWords);
  for (size_t b = 0; b < B; ++b) sbconv::mt_seed_python(&table[b * sbconv::kRngWords], seeds_host[b]);
  SB_ON_DEVICE(h->device);
  DevBuf<uint32_t> rng;
  if (!h->conv_rng.p) SB_CHECK(upload(rng, table.data(), table.size()));
  // the cell, partner and rank tables are the counter-based shuffle's: its attach builds them (and refuses what it refuses
  // before it changes anything); this mode then takes its place
  SB_CHECK(sb_convection_attach(h, p, distance, 0, 0, transposed));
  if (h->conv_rng.p) SB_HIP(hipMemcpy(h->conv_rng.p, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  else std::swap(h->conv_rng.p, rng.p);
  h->conv_attached = false;
  h->conv_seeded = true;
  h->conv_first = -1; // (sb_convection_attach sets it >= 0: see seeded_in_force)
  return SB_OK;
}

int sb_convection_rng_get(sb_handle *h, uint32_t *out_dev, void *stream) {
  if (!h || !out_dev) return fail(SB_ERR_INVALID, "sb_convection_rng_get: null argument");
  if (!seeded_in_force(h)) return fail(SB_ERR_INVALID, "sb_convection_rng_get: sb_convection_attach_seeded first");
  SB_ON_DEVICE(h->device);
  SB_HIP(hipMemcpyAsync(out_dev, h->conv_rng.p, (size_t)h->d.B * sbconv::kRngWords * sizeof(uint32_t),
                        hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SB_OK;
}

int sb_convection_rng_set(sb_handle *h, const uint32_t *in_dev, void *stream) {
  if (!h || !in_dev) return fail(SB_ERR_INVALID, "sb_convection_rng_set: null argument");
  if (!seeded_in_force(h)) return fail(SB_ERR_INVALID, "sb_convection_rng_set: sb_convection_attach_seeded first");
  SB_ON_DEVICE(h->device);
  SB_HIP(hipMemcpyAsync(h->conv_rng.p, in_dev, (size_t)h->d.B * sbconv::kRngWords * sizeof(uint32_t),
                        hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SB_OK;
}

int sb_convection_apply(sb_handle *h, void *stream) {
  if (!h) return fail(SB_ERR_INVALID, "sb_convection_apply: null handle");
  if (!h->conv_attached && !seeded_in_force(h))
    return fail(SB_ERR_INVALID, "sb_convection_apply: sb_convection_attach or sb_convection_attach_seeded first");
  SB_ON_DEVICE(h->device);
  return h->conv_attached ? sb_launch_convection(h, (hipStream_t)stream) : sb_launch_convection_seeded(h, (hipStream_t)stream);
}

} // extern "C"

int sb_launch_convection_seeded(sb_handle *h, hipStream_t stream) {
  const Dev &d = h->d;
  SeededArgs o;
  o.temp = d.temp; o.stride = d.reg ? (size_t)d.state_doubles : (size_t)d.Np;
  o.zone_off = h->zone_off.p; o.by_rank = h->conv_by_rank.p; o.cells = h->conv_cells.p; o.partner = h->conv_partner.p;
  o.rng = h->conv_rng.p;
  o.pw = h->conv_pw; o.B = d.B; o.Z = d.Z; o.max_room = h->conv_max_room; o.whole_room = h->conv_whole_room ? 1 : 0;
  o.p = h->conv_p;
  ++h->conv_calls;
  const size_t lds = seeded_lds_bytes(o.max_room); // what the kernel indexes: at most 31.6 KB (2047 cells)
  hipLaunchKernelGGL(k_convect_seeded, dim3(std::max(1, std::min(d.B, kSeededMaxWorkgroups))), dim3(kSeededThreads), lds,
                     stream, o);
  SB_HIP(hipGetLastError());
  return SB_OK;
}
