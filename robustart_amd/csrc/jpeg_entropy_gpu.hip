// Entropy decoding of a batch of baseline JPEG scans on gfx950: the self-synchronising parallel Huffman decoder of
// jpeg_entropy_par.h, one 256-thread workgroup per image, bit-identical to the sequential host decoder of jpeg_entropy.h.
//   k_jpeg_entropy : the image's Huffman tables (at most four, 1.5 KB each) are staged in LDS once; the threads step over the
//                    image's subsequences; the two exit tables (2 x 4096 packed 32-bit states) sit in LDS and one barrier
//                    (__syncthreads_or, which also carries "did any exit change") separates two rounds.  Then the per-subsequence
//                    records (blocks completed, DC sums) are prefix-summed in place -- each thread over a contiguous chunk, the
//                    256 chunk sums by one thread -- and the write pass stores the coefficients.
// Nothing waits across workgroups; rounds are bounded by max_rounds, a subsequence decode by its bits; every scan byte read is
// checked against the image's scan_len and every store against its block total (jpeg_entropy_par.h).  A corrupt file ends as a
// status word.
#include "rart_common.h"
#include "jpeg_entropy_par.h"

namespace {
using namespace rart_jpeg;
constexpr int kThreads = 256;
constexpr int kTableWords = kParTablePitch / 4;
static_assert(kParMaxSubseq == RART_JPEG_MAX_SUBSEQ && kParMaxTables == RART_JPEG_MAX_TABLES && kParTablePitch == RART_JPEG_HUFF_PITCH,
              "the header's limits are the decoder's");

__global__ __launch_bounds__(kThreads) void k_jpeg_entropy(const rart_jpeg_scan* __restrict__ desc, const uint8_t* __restrict__ scans,
                                                           const uint8_t* __restrict__ tabs, int16_t* __restrict__ coef,
                                                           int subseq_bytes, int max_rounds, int32_t* __restrict__ status,
                                                           int32_t* __restrict__ rounds_used, ParRecord* __restrict__ recs_all) {
  __shared__ uint32_t exits[2][kParMaxSubseq];
  __shared__ uint32_t tabmem[kParMaxTables * kTableWords];
  __shared__ ParImage I;
  __shared__ ParRecord part[kThreads + 1];
  __shared__ int bad;
  const int img = blockIdx.x, tid = threadIdx.x;
  const rart_jpeg_scan& d = desc[img];
  if (d.host_path) {   // the caller decoded it: uniform over the workgroup
    if (tid == 0) {
      status[img] = RART_OK;
      rounds_used[img] = 0;
    }
    return;
  }
  const int ntab = d.ntab < kParMaxTables ? d.ntab : kParMaxTables;
  const uint32_t* tsrc = reinterpret_cast<const uint32_t*>(tabs + d.tab_off);
  for (int i = tid; i < ntab * kTableWords; i += kThreads) tabmem[i] = tsrc[i];
  if (tid == 0) {
    I.scan = scans + d.scan_off;
    I.scan_len = d.scan_len;
    I.nsub = d.nsub < kParMaxSubseq ? d.nsub : kParMaxSubseq;
    I.subseq_bytes = subseq_bytes;
    I.ncomp = d.ncomp;
    I.hs = d.h_samp;
    I.vs = d.v_samp;
    I.nslots = d.ncomp == 1 ? 1 : d.h_samp * d.v_samp + 2;
    I.mcux = d.mcux;
    int start = 0;
    for (int c = 0; c < 3; ++c) {
      I.dc[c] = reinterpret_cast<const Huff*>(tabmem + (d.dc_tab[c] & 3) * kTableWords);
      I.ac[c] = reinterpret_cast<const Huff*>(tabmem + (d.ac_tab[c] & 3) * kTableWords);
      I.bw[c] = d.blocks_w[c];
      I.comp_start[c] = start;
      start += d.blocks_w[c] * d.blocks_h[c];
    }
    I.total_blocks = start;
    bad = 0;
  }
  __syncthreads();
  const int nsub = I.nsub;
  if (nsub <= 0) {   // no entropy-coded byte at all
    if (tid == 0) {
      status[img] = RART_ERR_INVALID;
      rounds_used[img] = 0;
    }
    return;
  }
  ParRecord* recs = recs_all + d.sub_start;
  int cur = 0, used = 0;
  bool converged = false;
  for (int round = 1; round <= max_rounds; ++round) {
    int any = 0;
    for (int t = tid; t < nsub; t += kThreads) {
      const uint32_t v = par_round(I, t, round, exits[cur ^ 1], &recs[t]);
      exits[cur][t] = v;
      any |= (int)(v >> 31);
    }
    cur ^= 1;
    used = round;
    if (!__syncthreads_or(any)) {
      converged = true;
      break;
    }
  }
  if (!converged) {
    if (tid == 0) {
      status[img] = RART_ERR_UNSUPPORTED;
      rounds_used[img] = used;
    }
    return;
  }
  const uint32_t* ex = exits[cur ^ 1];
  // exclusive prefix sums of the records, in place
  const int chunk = (nsub + kThreads - 1) / kThreads;
  const int lo = tid * chunk < nsub ? tid * chunk : nsub, hi = lo + chunk < nsub ? lo + chunk : nsub;
  ParRecord sum = {0, {0, 0, 0}, 0};
  for (int t = lo; t < hi; ++t) par_add(&sum, recs[t]);
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    ParRecord run = {0, {0, 0, 0}, 0};
    for (int i = 0; i < kThreads; ++i) {
      const ParRecord own = part[i];
      part[i] = run;
      par_add(&run, own);
    }
    part[kThreads] = run;
  }
  __syncthreads();
  ParRecord run = part[tid];
  for (int t = lo; t < hi; ++t) {
    const ParRecord own = recs[t];
    recs[t] = run;
    par_add(&run, own);
  }
  __syncthreads();
  int16_t* out = coef + d.block_start * 64;
  bool ok = true;
  for (int t = tid; t < nsub; t += kThreads) ok = par_write(I, t, t == 0 ? par_pack(0, 0, 0) : ex[t - 1], recs[t], out) && ok;
  if (!ok) bad = 1;
  __syncthreads();
  if (tid == 0) {
    status[img] = (bad || part[kThreads].blocks < (uint32_t)I.total_blocks) ? RART_ERR_INVALID : RART_OK;
    rounds_used[img] = used;
  }
}

// The host copy of the descriptors against the caller's buffers.  *first_gpu_block: where the coefficients the kernel writes begin.
int check_scans(const rart_jpeg_scan* d, int n, size_t scans_bytes, size_t tabs_bytes, long long total_blocks, int subseq_bytes,
                long long* total_sub, long long* first_gpu_block) {
  long long sub = 0, blk_end = 0;
  bool seen_gpu = false;
  *first_gpu_block = total_blocks;
  for (int i = 0; i < n; ++i) {
    const rart_jpeg_scan& e = d[i];
    RART_CHECK_ARG(e.ncomp == 1 || e.ncomp == 3, "rart_jpeg_entropy_decode_gpu: descriptor %d: ncomp must be 1 or 3", i);
    const bool samp_ok = e.ncomp == 1 ? (e.h_samp == 1 && e.v_samp == 1)
                                      : ((e.h_samp == 1 || e.h_samp == 2) && (e.v_samp == 1 || e.v_samp == 2) && e.h_samp >= e.v_samp);
    RART_CHECK_ARG(samp_ok, "rart_jpeg_entropy_decode_gpu: descriptor %d: luma sampling must be (1,1), (2,1) or (2,2)", i);
    RART_CHECK_ARG(e.mcux >= 1 && e.mcuy >= 1 && e.mcux <= 8192 && e.mcuy <= 8192 &&
                       (long long)e.mcux * e.mcuy * 64 * e.h_samp * e.v_samp <= kMaxPixels * 4,
                   "rart_jpeg_entropy_decode_gpu: descriptor %d: MCU grid out of range", i);
    long long blocks = 0;
    for (int c = 0; c < 3; ++c) {
      const int bw = c < e.ncomp ? (c == 0 ? e.mcux * e.h_samp : e.mcux) : 0, bh = c < e.ncomp ? (c == 0 ? e.mcuy * e.v_samp : e.mcuy) : 0;
      RART_CHECK_ARG(e.blocks_w[c] == bw && e.blocks_h[c] == bh, "rart_jpeg_entropy_decode_gpu: descriptor %d: block grid of component %d", i, c);
      blocks += (long long)bw * bh;
    }
    RART_CHECK_ARG(e.block_start >= blk_end && e.block_start + blocks <= total_blocks,
                   "rart_jpeg_entropy_decode_gpu: descriptor %d: blocks outside coef or overlapping the image before", i);
    blk_end = e.block_start + blocks;
    if (e.host_path) {
      RART_CHECK_ARG(!seen_gpu, "rart_jpeg_entropy_decode_gpu: descriptor %d: host-path images must come first", i);
      continue;
    }
    if (!seen_gpu) *first_gpu_block = e.block_start;
    seen_gpu = true;
    RART_CHECK_ARG(e.scan_len >= 0 && e.scan_len <= kParMaxScanBytes && e.scan_off >= 0 && (size_t)e.scan_off <= scans_bytes &&
                       (size_t)e.scan_len <= scans_bytes - (size_t)e.scan_off,
                   "rart_jpeg_entropy_decode_gpu: descriptor %d: scan bytes outside scans", i);
    RART_CHECK_ARG(e.nsub == (e.scan_len + subseq_bytes - 1) / subseq_bytes && e.nsub <= kParMaxSubseq,
                   "rart_jpeg_entropy_decode_gpu: descriptor %d: nsub does not match scan_len / subseq_bytes or exceeds %d", i, kParMaxSubseq);
    RART_CHECK_ARG(e.ntab >= 1 && e.ntab <= kParMaxTables && e.tab_off >= 0 && e.tab_off % 16 == 0 && (size_t)e.tab_off <= tabs_bytes &&
                       (size_t)e.ntab * kParTablePitch <= tabs_bytes - (size_t)e.tab_off,
                   "rart_jpeg_entropy_decode_gpu: descriptor %d: Huffman tables outside tabs", i);
    for (int c = 0; c < 3; ++c)
      RART_CHECK_ARG(e.dc_tab[c] >= 0 && e.dc_tab[c] < e.ntab && e.ac_tab[c] >= 0 && e.ac_tab[c] < e.ntab,
                     "rart_jpeg_entropy_decode_gpu: descriptor %d: table index of component %d", i, c);
    RART_CHECK_ARG(e.sub_start == sub, "rart_jpeg_entropy_decode_gpu: descriptor %d: sub_start must continue the numbering", i);
    sub += e.nsub;
  }
  *total_sub = sub;
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_jpeg_scan_plan(const uint8_t* data_host, size_t len, const rart_jpeg_info* info_host, int subseq_bytes,
                        rart_jpeg_scan* scan_host, void* tabs_host, size_t tabs_capacity) {
  RART_CHECK_ARG(data_host && info_host && scan_host, "rart_jpeg_scan_plan: null data / info / scan");
  if (subseq_bytes == 0) subseq_bytes = kParDefaultSubseq;
  RART_CHECK_ARG(par_subseq_ok(subseq_bytes), "rart_jpeg_scan_plan: subseq_bytes must be a power of two from 4 to 65536, got %d", subseq_bytes);
  Parsed P;
  const Result r = parse(data_host, len, &P);
  if (r.status != RART_OK) {
    rart_set_error("rart_jpeg_scan_plan: %s", r.why);
    return r.status;
  }
  rart_jpeg_info now;
  memset(&now, 0, sizeof(now));
  fill_info(P, &now);
  RART_CHECK_ARG(info_host->status == RART_OK && now.height == info_host->height && now.width == info_host->width &&
                     now.ncomp == info_host->ncomp && now.coef_count == info_host->coef_count,
                 "rart_jpeg_scan_plan: info does not describe this file (probe it first)");
  ParPlan pl;
  make_plan(data_host, len, P, subseq_bytes, &pl);
  fill_scan(P, now, pl, scan_host);
  if (!pl.host_path) {
    RART_CHECK_ARG(tabs_host && tabs_capacity >= (size_t)pl.ntab * kParTablePitch,
                   "rart_jpeg_scan_plan: tabs_host of %zu bytes required, got %zu", (size_t)pl.ntab * kParTablePitch, tabs_capacity);
    memset(tabs_host, 0, (size_t)pl.ntab * kParTablePitch);
    for (int j = 0; j < pl.ntab; ++j) memcpy((uint8_t*)tabs_host + (size_t)j * kParTablePitch, pl.tab[j], sizeof(Huff));
  }
  return RART_OK;
}

size_t rart_jpeg_entropy_workspace_bytes(const rart_jpeg_scan* scan_host, int n) {
  if (!scan_host || n <= 0) return 0;
  size_t sub = 0;
  for (int i = 0; i < n; ++i)
    if (!scan_host[i].host_path && scan_host[i].nsub > 0) sub += (size_t)scan_host[i].nsub;
  return rart_align_up(sub * sizeof(ParRecord) + 1, 256);
}

int rart_jpeg_entropy_decode_gpu(const rart_jpeg_scan* scan, const rart_jpeg_scan* scan_host, int n, const uint8_t* scans,
                                 size_t scans_bytes, const uint8_t* tabs, size_t tabs_bytes, int16_t* coef, int64_t total_blocks,
                                 int subseq_bytes, int max_rounds, int32_t* status, int32_t* rounds_used, void* workspace,
                                 size_t workspace_bytes, rart_stream_t stream) {
  RART_CHECK_ARG(n > 0, "rart_jpeg_entropy_decode_gpu: descriptor count must be positive, got %d", n);
  RART_CHECK_ARG(scan && scan_host && scans && tabs && coef && status && rounds_used && total_blocks > 0,
                 "rart_jpeg_entropy_decode_gpu: bad arguments (a null pointer or no blocks)");
  if (subseq_bytes == 0) subseq_bytes = kParDefaultSubseq;
  if (max_rounds == 0) max_rounds = kParDefaultRounds;
  RART_CHECK_ARG(par_subseq_ok(subseq_bytes), "rart_jpeg_entropy_decode_gpu: subseq_bytes must be a power of two from 4 to 65536, got %d",
                 subseq_bytes);
  RART_CHECK_ARG(max_rounds > 0, "rart_jpeg_entropy_decode_gpu: max_rounds must not be negative");
  RART_CHECK_ARG(((uintptr_t)scan & 7) == 0 && ((uintptr_t)tabs & 15) == 0 && ((uintptr_t)coef & 15) == 0 && ((uintptr_t)status & 3) == 0 &&
                     ((uintptr_t)rounds_used & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
                 "rart_jpeg_entropy_decode_gpu: tabs, coef and the workspace must be 16-byte aligned, scan 8-byte, status / rounds_used 4-byte");
  long long total_sub = 0, first = 0;
  const int st = check_scans(scan_host, n, scans_bytes, tabs_bytes, total_blocks, subseq_bytes, &total_sub, &first);
  if (st != RART_OK) return st;
  const size_t need = rart_align_up((size_t)total_sub * sizeof(ParRecord) + 1, 256);
  if (!workspace || workspace_bytes < need) {
    rart_set_error("rart_jpeg_entropy_decode_gpu: workspace of %zu bytes required, got %zu", need, workspace_bytes);
    return RART_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (first < total_blocks) {
    const hipError_t e = hipMemsetAsync(coef + first * 64, 0, (size_t)(total_blocks - first) * 128, s);
    if (e != hipSuccess) {
      rart_set_error("rart_jpeg_entropy_decode_gpu (memset): %s", hipGetErrorString(e));
      return RART_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(k_jpeg_entropy, dim3((unsigned)n), dim3(kThreads), 0, s, scan, scans, tabs, coef, subseq_bytes, max_rounds, status,
                     rounds_used, (ParRecord*)workspace);
  RART_CHECK_LAUNCH("rart_jpeg_entropy_decode_gpu");
  return RART_OK;
}

int rart_jpeg_entropy_emulate(const uint8_t* data_host, size_t len, const rart_jpeg_info* info_host, int subseq_bytes,
                              int max_rounds, int16_t* coef_host, size_t capacity, int32_t* rounds_used) {
  int used = 0;
  const Result r = emulate(data_host, len, info_host, subseq_bytes, max_rounds, coef_host, capacity, rounds_used ? &used : nullptr);
  if (rounds_used) *rounds_used = used;
  if (r.status != RART_OK) rart_set_error("rart_jpeg_entropy_emulate: %s", r.why);
  return r.status;
}

}  // extern "C"
