// Earth mover's distance between two clouds of n points each (n <= 8192): an exact, bitwise repeatable linear assignment by a
// forward auction in Jacobi form with eps-scaling, all in int64 (nm_emd, include/neuma_hip.h; the numpy twin that reproduces
// assignment, prices and round count bit for bit is neuma_amd/extras/emd.py; derivation and numbers in DESIGN.md section 7).
//
// One workgroup per batch item runs the whole auction in ONE launch: a `for (round < max_rounds)` loop with workgroup barriers
// between the bid half, the award half and the compaction of the unassigned persons.  No cooperative launch, no grid-wide
// barrier, no waiting on another workgroup; every loop is bounded by n, by a list length <= n or by max_rounds.
//
// LDS per item (dynamic, sized by n; 149,504 bytes at n = 8192, one workgroup per CU there):
//   P[n]     u64   price << 13 | (8191 - owner): the price snapshot every bidder of a round reads, and the owner of the object
//   bid[n]   u64   this round's bids, packed the same way (0 = none); one ds_max_u64 per bidder.  The maximum of the packed
//                  word is the highest bid and, among equal bids, the lowest person - whatever order the waves arrive in.
//   assigned, owned   one bit per person / per object (owned: P's owner field is of this phase)
//   list[n]  u16   the unassigned persons, ascending
// The coordinates (2 x 12 n bytes, read once per cost evaluation) stay in global memory / L2; costs are recomputed for every
// evaluation, there is no n x n matrix anywhere.
#include <limits.h>
#include <math.h>

#include <vector>

#include "nm_common.h"
#include "nm_reduce.h"
#include "nm_workspace.h"

namespace {

constexpr int kEmdMaxN = 8192;
constexpr int kEmdBits = 24;                      // C <= 2^24
constexpr int kPersonBits = 13;                   // 8192 persons
constexpr unsigned long long kPersonMask = (1ull << kPersonBits) - 1;
constexpr long long kBidLimit = 1ll << 50;        // a bid must pack into 63 bits next to the person

enum { EMD_DONE = 0, EMD_NONFINITE = 1, EMD_ROUND_LIMIT = 2, EMD_OVERFLOW = 3 };

// c(i,j) = (dx*dx + dy*dy) + dz*dz in fp64 from the fp32 coordinates (this file is compiled with -ffp-contract=off); power 1 takes
// the fp64 square root, which is correctly rounded
template <int POWER>
__device__ __forceinline__ double emd_cost(double ax, double ay, double az, const float* __restrict__ q) {
  const double dx = ax - (double)q[0], dy = ay - (double)q[1], dz = az - (double)q[2];
  const double c = (dx * dx + dy * dy) + dz * dz;
  return POWER == 1 ? sqrt(c) : c;
}
// C = llrint(ldexp(c, k)); 0 <= C <= 2^24, so the rounded value converts through int32
__device__ __forceinline__ unsigned emd_quantise(double c, int k) { return (unsigned)__double2int_rn(ldexp(c, k)); }

// A bidder maximises v_j = -Cs(i,j) - price_j; the kernel carries u_j = -v_j = Cs(i,j) + price_j >= 0 (one 32 x 32 + 64 bit
// multiply-add) and minimises it: the smallest u with the lowest object of that u, and the smallest u among all OTHER objects.
// w1 - w2 = u2 - u1.
struct EmdBest {
  unsigned long long u1;
  int j1;
  unsigned long long u2;
};
constexpr unsigned long long kEmdNone = ~0ull;
__device__ __forceinline__ void emd_take(EmdBest& best, unsigned long long u, int j) {
  if (u < best.u1) {          // ascending j: a later equal value does not replace the lowest j
    best.u2 = best.u1;
    best.u1 = u;
    best.j1 = j;
  } else if (u < best.u2) {
    best.u2 = u;
  }
}
__device__ __forceinline__ EmdBest emd_merge(const EmdBest& a, const EmdBest& b) {
  const bool a_first = a.u1 < b.u1 || (a.u1 == b.u1 && a.j1 < b.j1);
  const unsigned long long loser = a_first ? b.u1 : a.u1, second = a_first ? a.u2 : b.u2;
  EmdBest r;
  r.u1 = a_first ? a.u1 : b.u1;
  r.j1 = a_first ? a.j1 : b.j1;
  r.u2 = second < loser ? second : loser;
  return r;
}

constexpr int kEmdBatch = 4;
__device__ __forceinline__ void emd_load_batch(float (&q)[kEmdBatch][3], const float* __restrict__ b, int j, int n) {
#pragma unroll
  for (int t = 0; t < kEmdBatch; ++t) {
    const int jj = j + 64 * t < n ? j + 64 * t : n - 1;
    q[t][0] = b[3 * (size_t)jj];
    q[t][1] = b[3 * (size_t)jj + 1];
    q[t][2] = b[3 * (size_t)jj + 2];
  }
}

// bid = price_j* + (w1 - w2) + eps, posted as one LDS maximum of bid << 13 | (8191 - person); a bid of 2^50 or more does not
// pack and ends the item ("price overflow")
__device__ __forceinline__ void emd_post_bid(const EmdBest& best, int i, int n, long long eps, const unsigned long long* P,
                                             unsigned long long* bid, long long* s_ctl) {
  const long long gap = n > 1 ? (long long)(best.u2 - best.u1) : 0;       // w1 - w2
  const long long value = (long long)(P[best.j1] >> kPersonBits) + gap + eps;
  if (value >= kBidLimit) s_ctl[2] = 2;
  else atomicMax(&bid[best.j1], ((unsigned long long)value << kPersonBits) | (unsigned long long)(kEmdMaxN - 1 - i));
}

// a sum carried as value + error (two-sum), so that the mean is the exact sum's rounding to within an ulp whatever n is
struct EmdSum {
  double s, e;
};
__device__ __forceinline__ EmdSum emd_add(const EmdSum& a, const EmdSum& b) {
  const double s = a.s + b.s, bb = s - a.s;
  const double err = (a.s - (s - bb)) + (b.s - bb);
  const double e = err + (a.e + b.e);
  EmdSum r;
  r.s = s + e;
  r.e = e - (r.s - s);
  return r;
}

__device__ __forceinline__ void emd_fail_outputs(int n, int64_t* idx, double* emd_out, int64_t* rounds_out, int64_t rounds) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) idx[i] = -1;
  if (threadIdx.x == 0) {
    *emd_out = __builtin_nan("");
    *rounds_out = rounds;
  }
}

template <int NW, int POWER>
__global__ __launch_bounds__(NW * 64) void k_emd(int n, long long max_rounds, const float* __restrict__ a_all,
                                                 const float* __restrict__ b_all, double* __restrict__ emd_out,
                                                 int64_t* __restrict__ idx_all, int64_t* __restrict__ price_all,
                                                 int64_t* __restrict__ rounds_out, int* __restrict__ status) {
  constexpr int T = NW * 64;
  extern __shared__ __align__(16) unsigned char emd_lds[];
  __shared__ float sh_box[NW * 8];
  __shared__ double sh_sum[NW * 2];
  __shared__ long long sh_max[NW];
  __shared__ unsigned long long sh_part[NW * 3];     // a bidder's partial results when several waves share it
  __shared__ long long s_ctl[4];      // eps, number of unassigned persons, state (0 running, 1 done, 2 price overflow)

  const int item = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwords = (n + 31) >> 5;
  unsigned long long* P = (unsigned long long*)emd_lds;
  unsigned long long* bid = P + n;
  uint32_t* assigned = (uint32_t*)(bid + n);
  uint32_t* owned = assigned + nwords;
  uint16_t* list = (uint16_t*)(owned + nwords);

  const float* __restrict__ a = a_all + (size_t)item * n * 3;
  const float* __restrict__ b = b_all + (size_t)item * n * 3;
  int64_t* idx = idx_all + (size_t)item * n;
  int64_t* price_out = price_all ? price_all + (size_t)item * n : nullptr;

  // ---- joint bounding box, and whether every coordinate is finite
  float box[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.f};
  for (int t = tid; t < 2 * n; t += T) {
    const float* q = t < n ? a + 3 * (size_t)t : b + 3 * (size_t)(t - n);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = q[d];
      box[d] = fminf(box[d], v);
      box[3 + d] = fmaxf(box[3 + d], v);
      if (!(fabsf(v) <= 3.402823466e+38f)) box[6] = 1.f;
    }
  }
  const auto tot = nm_block_reduce<NW, NmMinMax<3>>(box, sh_box);
  if (tot[6] != 0.f) {
    emd_fail_outputs(n, idx, emd_out + item, rounds_out + item, 0);
    if (price_out)
      for (int j = tid; j < n; j += T) price_out[j] = 0;
    if (tid == 0) status[item] = EMD_NONFINITE;
    return;
  }
  const double ex = (double)tot[3] - (double)tot[0], ey = (double)tot[4] - (double)tot[1], ez = (double)tot[5] - (double)tot[2];
  const double c_ext = (ex * ex + ey * ey) + ez * ez;
  const double cmax = POWER == 1 ? sqrt(c_ext) : c_ext;
  if (cmax == 0.0) {      // all points identical: the identity, EMD 0, no rounds
    for (int i = tid; i < n; i += T) {
      idx[i] = i;
      if (price_out) price_out[i] = 0;
    }
    if (tid == 0) {
      emd_out[item] = 0.0;
      rounds_out[item] = 0;
      status[item] = EMD_DONE;
    }
    return;
  }
  int exponent;
  frexp(cmax, &exponent);
  const int kq = kEmdBits - exponent;
  const long long np1 = (long long)n + 1;
  const unsigned np1u = (unsigned)n + 1u;

  // ---- eps0 = max(1, max(Cs) / 2): one pass over all pairs
  long long cbig = 0;
  for (int i = wave; i < n; i += NW) {
    const double ax = a[3 * (size_t)i], ay = a[3 * (size_t)i + 1], az = a[3 * (size_t)i + 2];
#pragma unroll 4
    for (int j = lane; j < n; j += 64) {
      const long long c = emd_quantise(emd_cost<POWER>(ax, ay, az, b + 3 * (size_t)j), kq);
      cbig = c > cbig ? c : cbig;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long other = __shfl_xor(cbig, o, 64);
    cbig = other > cbig ? other : cbig;
  }
  if (lane == 0) sh_max[wave] = cbig;
  for (int j = tid; j < n; j += T) {
    P[j] = 0;
    bid[j] = 0;
    list[j] = (uint16_t)j;
  }
  for (int w = tid; w < nwords; w += T) {
    assigned[w] = 0;
    owned[w] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    long long m = sh_max[0];
    for (int w = 1; w < NW; ++w) m = sh_max[w] > m ? sh_max[w] : m;
    const long long eps0 = (m * np1) / 2;
    s_ctl[0] = eps0 > 1 ? eps0 : 1;
    s_ctl[1] = n;
    s_ctl[2] = 0;
  }
  __syncthreads();

  // ---- the auction
  long long rounds = -1;
  int state = 0;
  for (long long round = 0; round < max_rounds; ++round) {
    const int count = (int)s_ctl[1];
    const long long eps = s_ctl[0];
    // bid half: every unassigned person bids from the same snapshot P.  A wave per bidder, its lanes striding over the objects;
    // when there are fewer bidders than waves (the long tail of every phase), `split` waves share a bidder, each taking a
    // slice of the objects, and one thread per bidder merges their partial results.  The merge is a minimum in a total
    // order (u, then lowest object), so the split changes no bit of the outcome.
    int split = 1;
    while (split * 2 * count <= NW) split *= 2;
    const int slice = ((n + split * 64 - 1) / (split * 64)) * 64;
    for (int u = wave; u < count * split; u += NW) {
      const int k = u / split, part = u - k * split;
      const int i = list[k];
      const int j_end = (part + 1) * slice < n ? (part + 1) * slice : n;
      const double ax = a[3 * (size_t)i], ay = a[3 * (size_t)i + 1], az = a[3 * (size_t)i + 2];
      EmdBest best = {kEmdNone, INT_MAX, kEmdNone};
      // kEmdBatch objects per lane at a time, the next batch's coordinates in flight while this one is evaluated (a load
      // past the slice's end reads point n - 1 and is not used)
      float cur[kEmdBatch][3], nxt[kEmdBatch][3];
      int j = part * slice + lane;
      emd_load_batch(cur, b, j, n);
      for (; j < j_end; j += 64 * kEmdBatch) {
        emd_load_batch(nxt, b, j + 64 * kEmdBatch, n);
#pragma unroll
        for (int t = 0; t < kEmdBatch; ++t) {
          const int jj = j + 64 * t;
          if (jj < j_end) {
            const unsigned c = emd_quantise(emd_cost<POWER>(ax, ay, az, cur[t]), kq);
            emd_take(best, (unsigned long long)c * np1u + (P[jj] >> kPersonBits), jj);
          }
        }
#pragma unroll
        for (int t = 0; t < kEmdBatch; ++t) {
          cur[t][0] = nxt[t][0];
          cur[t][1] = nxt[t][1];
          cur[t][2] = nxt[t][2];
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        EmdBest other;
        other.u1 = __shfl_xor(best.u1, o, 64);
        other.j1 = __shfl_xor(best.j1, o, 64);
        other.u2 = __shfl_xor(best.u2, o, 64);
        best = emd_merge(best, other);
      }
      if (lane == 0) {
        if (split == 1) {
          emd_post_bid(best, i, n, eps, P, bid, s_ctl);
        } else {            // (count * split <= NW: u is this wave's only unit)
          sh_part[3 * u] = best.u1;
          sh_part[3 * u + 1] = (unsigned long long)best.j1;
          sh_part[3 * u + 2] = best.u2;
        }
      }
    }
    if (split > 1) {
      __syncthreads();
      if (tid < count) {
        EmdBest best = {sh_part[3 * tid * split], (int)sh_part[3 * tid * split + 1], sh_part[3 * tid * split + 2]};
        for (int g = 1; g < split; ++g) {
          const unsigned long long* q = sh_part + 3 * (tid * split + g);
          const EmdBest other = {q[0], (int)q[1], q[2]};
          best = emd_merge(best, other);
        }
        emd_post_bid(best, list[tid], n, eps, P, bid, s_ctl);
      }
    }
    __syncthreads();
    if (s_ctl[2] == 2) {
      state = 2;
      break;
    }
    // award half: the packed maximum is the winner; it takes the object, the previous owner of this phase becomes unassigned
    for (int j = tid; j < n; j += T) {
      const unsigned long long won = bid[j];
      if (won != 0) {
        const uint32_t bit = 1u << (j & 31);
        if (owned[j >> 5] & bit) {
          const int q = kEmdMaxN - 1 - (int)(P[j] & kPersonMask);
          atomicAnd(&assigned[q >> 5], ~(1u << (q & 31)));
        } else {
          atomicOr(&owned[j >> 5], bit);
        }
        const int w = kEmdMaxN - 1 - (int)(won & kPersonMask);
        atomicOr(&assigned[w >> 5], 1u << (w & 31));
        P[j] = won;
        bid[j] = 0;
      }
    }
    __syncthreads();
    // compaction by wave 0: lane l lists the unassigned persons of its (at most 4) consecutive mask words, in ascending order
    if (wave == 0) {
      const int per_lane = (nwords + 63) >> 6;
      const int w0 = lane * per_lane;
      uint32_t m[4];
      int mine = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int w = w0 + t;
        uint32_t un = 0;
        if (t < per_lane && w < nwords) {
          un = ~assigned[w];
          if (w == nwords - 1 && (n & 31)) un &= (1u << (n & 31)) - 1u;
        }
        m[t] = un;
        mine += __popc(un);
      }
      int incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      const int unassigned = __shfl(incl, 63, 64);
      const long long eps_now = s_ctl[0];
      long long next_eps = eps_now;
      int next_count = unassigned, finished = 0;
      if (unassigned > 0) {
        int pos = incl - mine;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          uint32_t un = m[t];
          for (int s = 0; s < 32 && un != 0; ++s) {
            list[pos++] = (uint16_t)(((w0 + t) << 5) + __ffs((int)un) - 1);
            un &= un - 1u;
          }
        }
      } else if (eps_now > 1) {     // next phase: nobody assigned, the prices stay
        for (int w = lane; w < nwords; w += 64) {
          assigned[w] = 0;
          owned[w] = 0;
        }
        for (int i = lane; i < n; i += 64) list[i] = (uint16_t)i;
        next_count = n;
        next_eps = eps_now / 4 > 1 ? eps_now / 4 : 1;
      } else {
        finished = 1;
      }
      if (lane == 0) {
        s_ctl[0] = next_eps;
        s_ctl[1] = next_count;
        if (finished) s_ctl[2] = 1;
      }
    }
    __syncthreads();
    if (s_ctl[2] == 1) {
      state = 1;
      rounds = round + 1;
      break;
    }
  }

  // ---- outputs
  if (price_out)
    for (int j = tid; j < n; j += T) price_out[j] = (int64_t)(P[j] >> kPersonBits);
  if (state != 1) {       // round limit or price overflow: NaN, -1, rounds -1; the host turns the status into an error
    emd_fail_outputs(n, idx, emd_out + item, rounds_out + item, -1);
    if (tid == 0) status[item] = state == 2 ? EMD_OVERFLOW : EMD_ROUND_LIMIT;
    return;
  }
  EmdSum sum = {0.0, 0.0};
  for (int j = tid; j < n; j += T) {
    const int i = kEmdMaxN - 1 - (int)(P[j] & kPersonMask);
    idx[i] = j;
    const EmdSum term = {emd_cost<POWER>(a[3 * (size_t)i], a[3 * (size_t)i + 1], a[3 * (size_t)i + 2], b + 3 * (size_t)j), 0.0};
    sum = emd_add(sum, term);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    EmdSum other;
    other.s = __shfl_xor(sum.s, o, 64);
    other.e = __shfl_xor(sum.e, o, 64);
    // (both lanes of a pair must add in the same order to hold the same bits)
    sum = (lane & o) ? emd_add(other, sum) : emd_add(sum, other);
  }
  if (lane == 0) {
    sh_sum[2 * wave] = sum.s;
    sh_sum[2 * wave + 1] = sum.e;
  }
  __syncthreads();
  if (tid == 0) {
    EmdSum all = {sh_sum[0], sh_sum[1]};
    for (int w = 1; w < NW; ++w) {
      const EmdSum part = {sh_sum[2 * w], sh_sum[2 * w + 1]};
      all = emd_add(all, part);
    }
    emd_out[item] = all.s / (double)n;
    rounds_out[item] = rounds;
    status[item] = EMD_DONE;
  }
}

size_t emd_lds_bytes(int n) {
  const size_t nwords = ((size_t)n + 31) / 32;
  return ((size_t)n * (8 + 8 + 2) + nwords * 8 + 15) & ~(size_t)15;
}

template <int NW, int POWER>
int emd_launch(int32_t b, int32_t n, int64_t max_rounds, const float* pa, const float* pb, double* emd_out,
               int64_t* idx_out, int64_t* price_out, int64_t* rounds_out, int* status, hipStream_t s) {
  static bool attr_set[64] = {};       // (a function attribute belongs to the device it was set on; one flag set per instance)
  int devid = 0;
  NM_HIP_CHECK(hipGetDevice(&devid));
  if (devid < 0 || devid >= 64 || !attr_set[devid]) {
    NM_HIP_CHECK(hipFuncSetAttribute((const void*)k_emd<NW, POWER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)emd_lds_bytes(kEmdMaxN)));
    if (devid >= 0 && devid < 64) attr_set[devid] = true;
  }
  NM_LAUNCH((k_emd<NW, POWER>), dim3(b), dim3(NW * 64), emd_lds_bytes(n), s, n, (long long)max_rounds, pa, pb, emd_out, idx_out,
            price_out, rounds_out, status);
  NM_LAUNCH_CHECK();
  return NM_OK;
}

}  // namespace

extern "C" size_t nm_emd_workspace(int32_t b, int32_t n) {
  if (b < 1 || b > 65535 || n < 1 || n > kEmdMaxN) return 0;
  NmCarver c(nullptr);
  c.take<int>((size_t)b);
  return c.total();
}

extern "C" int nm_emd(int32_t b, int32_t n, int32_t power, int64_t max_rounds, const float* pa, const float* pb, double* emd_out,
                      int64_t* idx_out, int64_t* price_out, int64_t* rounds_out, void* ws, size_t ws_bytes, void* stream) {
  NM_REQUIRE(b >= 1 && b <= 65535, "b must be in [1, 65535]");
  NM_REQUIREF(n >= 1 && n <= kEmdMaxN, "n must be in [1, %d], got %d", kEmdMaxN, n);
  NM_REQUIREF(power == 1 || power == 2, "power must be 1 or 2, got %d", power);
  NM_REQUIRE(max_rounds >= 1, "max_rounds must be at least 1");
  NM_REQUIRE(pa && pb && emd_out && idx_out && rounds_out && ws, "null pointer");
  NM_REQUIRE(ws_bytes >= nm_emd_workspace(b, n), "workspace too small (nm_emd_workspace)");
  const hipStream_t s = (hipStream_t)stream;
  NmCarver c(ws);
  int* status = c.take<int>((size_t)b);
  // 16 waves where there is work for them: more bidders per round in flight; small clouds pay less per barrier with 4
  const bool wide = n > 512;
  const int rc = power == 1 ? (wide ? emd_launch<16, 1>(b, n, max_rounds, pa, pb, emd_out, idx_out, price_out, rounds_out, status, s)
                                    : emd_launch<4, 1>(b, n, max_rounds, pa, pb, emd_out, idx_out, price_out, rounds_out, status, s))
                            : (wide ? emd_launch<16, 2>(b, n, max_rounds, pa, pb, emd_out, idx_out, price_out, rounds_out, status, s)
                                    : emd_launch<4, 2>(b, n, max_rounds, pa, pb, emd_out, idx_out, price_out, rounds_out, status, s));
  if (rc != NM_OK) return rc;
  // the status words are the one thing read back: this synchronises the stream
  std::vector<int> host((size_t)b);
  NM_HIP_CHECK(hipMemcpyAsync(host.data(), status, (size_t)b * sizeof(int), hipMemcpyDeviceToHost, s));
  NM_HIP_CHECK(hipStreamSynchronize(s));
  for (int32_t i = 0; i < b; ++i) {
    if (host[i] == EMD_ROUND_LIMIT) {
      nm_set_error("nm_emd: item %d reached the round limit (max_rounds = %lld) before every point was assigned", i,
                   (long long)max_rounds);
      return NM_ERR_LIMIT;
    }
    if (host[i] == EMD_OVERFLOW) {
      nm_set_error("nm_emd: item %d: price overflow (a bid reached 2^50)", i);
      return NM_ERR_LIMIT;
    }
  }
  return NM_OK;
}
