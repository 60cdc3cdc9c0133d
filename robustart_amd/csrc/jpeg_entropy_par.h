// Self-synchronising parallel Huffman decoding of one baseline scan ("Entropy decoding on the device"), written
// once for the host (rart_jpeg_entropy_emulate, tests/host/jpeg_entropy_par_fuzz.cpp) and for the device
// (csrc/jpeg_entropy_gpu.hip).  The scheme of Weissenberger & Schmidt, restricted so that the result is the sequential decoder's
// (jpeg_entropy.h) or a status word, never a guess:
//
//   * The entropy-coded segment [scan_pos, stop) is cut into subsequences of `subseq_bytes` raw bytes.  The decoder's state between
//     two symbols is (bit position, block slot inside the MCU, zigzag index k; k = 0: a DC code comes next), packed in 32 bits.
//     A bit position counts raw bits from scan_pos and never stands inside a stuffed 00.
//   * Subsequence t owns the symbols that START inside it; the state at which its decode leaves its range is its exit, the entry
//     of t + 1.  Round 1 decodes every subsequence from a guess (its first bit -- the byte after it when it starts on the 00 of an
//     FF 00 -- slot 0, k 0), subsequence 0 from the true state.  Round r > 1 decodes again every subsequence whose predecessor's
//     exit changed in round r - 1, from that exit; a round reads only what the round before wrote (two exit tables), so the number
//     of rounds is a function of the file and subseq_bytes alone.  A round that changes no exit ends the loop: by induction over t
//     every exit is then the sequential decoder's.  After max_rounds rounds without that the image is RART_ERR_UNSUPPORTED.
//   * Error rule.  A decode that meets bits no code starts, a code or its extra bits running past `stop`, a DC category above 11,
//     an AC category above 10 or a coefficient index past 63 consumes ONE bit, goes to slot 0, k 0 and carries on.  Every step
//     consumes at least one bit, so a subsequence takes at most 8 subseq_bytes steps.
//   * Every decode of a subsequence also counts the blocks it completes and sums, per component, the DC differences it owns
//     (mod 2^16: the sequential decoder keeps the predictor in uint32 and stores int16).  Exclusive prefix sums over the
//     subsequences give each one its first scan-order block and its predictors.
//   * The write pass decodes every subsequence once more from its true entry and stores the coefficients of blocks below the image's
//     block total.  An error the true chain meets below the total, or a chain that ends below it, is RART_ERR_INVALID -- exactly
//     where the sequential decoder returns it; what follows the last block is ignored, as there.
#pragma once
#include <stdlib.h>

#include "jpeg_entropy.h"

namespace rart_jpeg {

constexpr int kParMaxSubseq = 4096;                 // exits of one image held at once (two tables of 32-bit states)
constexpr int kParMaxScanBytes = (1 << 19) - 2;     // bit positions fit the state's 22 bits
constexpr int kParMaxTables = 4;                    // distinct Huffman tables of one image
constexpr int kParTablePitch = 1504;                // sizeof(Huff) rounded up to 16
constexpr int kParDefaultSubseq = RART_JPEG_DEFAULT_SUBSEQ_BYTES;
constexpr int kParDefaultRounds = RART_JPEG_DEFAULT_MAX_ROUNDS;
static_assert(sizeof(Huff) <= kParTablePitch, "table pitch");

constexpr uint32_t kParChanged = 0x80000000u;       // flag of an exit-table entry: this exit changed in the round that wrote it
constexpr uint32_t kParState = 0x7FFFFFFFu;

RART_JPEG_HD inline uint32_t par_pack(uint32_t pos, int slot, int k) { return (pos << 9) | ((uint32_t)slot << 6) | (uint32_t)k; }
RART_JPEG_HD inline uint32_t par_pos(uint32_t st) { return (st & kParState) >> 9; }
RART_JPEG_HD inline int par_slot(uint32_t st) { return (int)((st >> 6) & 7u); }
RART_JPEG_HD inline int par_k(uint32_t st) { return (int)(st & 63u); }

RART_JPEG_HD inline int par_natural(int k) {
  constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return nat[k & 63];
}

// One image as the decode steps see it.  scan: the scan_len bytes [scan_pos, stop); every FF in it is followed by its 00.
struct ParImage {
  const uint8_t* scan;
  const Huff* dc[3];
  const Huff* ac[3];
  int scan_len, nsub, subseq_bytes;
  int ncomp, hs, vs, nslots;       // luma's sampling factors (chroma is (1,1)); blocks per MCU
  int mcux, total_blocks;
  int bw[3];
  int comp_start[3];               // the component's first block inside the image's coefficients
};

struct ParRecord {                 // of one subsequence's latest decode; after par_prefix: what precedes the subsequence
  uint32_t blocks;
  uint16_t dc[3];
  uint16_t pad_;
};

RART_JPEG_HD inline int par_comp_of_slot(const ParImage& I, int slot) {
  const int luma = I.hs * I.vs;
  return slot < luma ? 0 : slot - luma + 1;
}

// scan-order block B (< total_blocks) -> its first coefficient inside the image: (MCU, slot) -> (component, block row, block column)
RART_JPEG_HD inline int par_block_addr(const ParImage& I, int B) {
  const int mcu = B / I.nslots, slot = B - mcu * I.nslots;
  const int my = mcu / I.mcux, mx = mcu - my * I.mcux;
  const int luma = I.hs * I.vs;
  if (slot < luma) {
    const int v = slot / I.hs, h = slot - v * I.hs;
    return (I.comp_start[0] + (my * I.vs + v) * I.bw[0] + mx * I.hs + h) * 64;
  }
  const int c = slot - luma + 1;
  return (I.comp_start[c] + my * I.bw[c] + mx) * 64;
}

enum { kParNone = 0, kParDC = 1, kParAC = 2, kParError = 3 };
struct ParEvent {
  int kind, comp, k, value;
  bool block_done;
};

// One step from *st (a bit position below 8 scan_len): the code there and its extra bits, or the error rule.  -> the event; *st
// moves on by at least one bit.
RART_JPEG_HD inline ParEvent par_step(const ParImage& I, uint32_t* st) {
  const uint32_t pos = par_pos(*st);
  int slot = par_slot(*st), k = par_k(*st);
  if (slot >= I.nslots) slot = 0;
  const int o = (int)(pos & 7u);
  // a window of up to five data bytes (a code of 16 bits + 11 extra bits + 7 bits of offset = 34 bits at the most)
  int rp[5];
  uint64_t win = 0;
  int got = 0, rr = (int)(pos >> 3);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    rp[i] = rr;
    if (rr >= 0 && rr < I.scan_len) {
      const uint8_t b = I.scan[rr];
      rr += b == 0xFF ? 2 : 1;
      if (rr > I.scan_len) rr = I.scan_len;
      win |= (uint64_t)b << (32 - 8 * i);
      got += 8;
    }
  }
  const int avail = got - o;
  const uint64_t w = win << (24 + o);
  const int c = par_comp_of_slot(I, slot);
  ParEvent ev = {kParNone, c, 0, 0, false};
  int sym = 0, used = 0;
  bool ok = true;
  if (k == 0) {
    const int l = huff_lookup(*I.dc[c], (uint32_t)(w >> 48), &sym);
    if (!l || l > avail || sym > 11 || l + sym > avail) {
      ok = false;
    } else {
      ev.kind = kParDC;
      ev.value = sym ? extend((uint32_t)((w << l) >> (64 - sym)), sym) : 0;
      used = l + sym;
      k = 1;
    }
  } else {
    const int l = huff_lookup(*I.ac[c], (uint32_t)(w >> 48), &sym);
    const int run = sym >> 4, s = sym & 15;
    if (!l || l > avail) {
      ok = false;
    } else if (s == 0) {
      used = l;
      if (run != 15) ev.block_done = true;   // end of block
      else k += 16;                          // ZRL
    } else if (s > 10 || k + run > 63 || l + s > avail) {
      ok = false;
    } else {
      ev.kind = kParAC;
      ev.k = k + run;
      ev.value = extend((uint32_t)((w << l) >> (64 - s)), s);
      used = l + s;
      k = k + run + 1;
    }
    if (ok && k > 63) ev.block_done = true;
  }
  if (!ok) {
    ev.kind = kParError;
    ev.block_done = false;
    used = 1;
    slot = 0;
    k = 0;
  } else if (ev.block_done) {
    k = 0;
    slot = slot + 1 == I.nslots ? 0 : slot + 1;
  }
  const int tot = o + used;   // <= 34: lands in window byte 0..4
  int at = rp[0];
#pragma unroll
  for (int i = 1; i < 5; ++i)
    if ((tot >> 3) >= i) at = rp[i];
  *st = par_pack((uint32_t)at * 8u + (uint32_t)(tot & 7), slot, k);
  return ev;
}

// The guessed entry of subsequence t >= 1.
RART_JPEG_HD inline uint32_t par_guess(const ParImage& I, int t) {
  int s = t * I.subseq_bytes;
  if (s > 0 && s < I.scan_len && I.scan[s - 1] == 0xFF && I.scan[s] == 0) ++s;
  return par_pack((uint32_t)s * 8u, 0, 0);
}

// Decodes subsequence t from `entry`: every symbol that starts below the subsequence's last bit goes to sink(event) (return false
// to stop early).  -> the exit.
template <class Sink>
RART_JPEG_HD inline uint32_t par_decode(const ParImage& I, int t, uint32_t entry, Sink& sink) {
  int end = (t + 1) * I.subseq_bytes;
  if (end > I.scan_len) end = I.scan_len;
  const uint32_t end_bits = (uint32_t)end * 8u;
  uint32_t st = entry & kParState;
  for (int it = 0; it < 8 * I.subseq_bytes && par_pos(st) < end_bits; ++it) {
    const ParEvent ev = par_step(I, &st);
    if (!sink(ev)) break;
  }
  return st;
}

struct ParCount {
  ParRecord r = {0, {0, 0, 0}, 0};
  RART_JPEG_HD bool operator()(const ParEvent& ev) {
    if (ev.kind == kParDC) {
#pragma unroll
      for (int c = 0; c < 3; ++c)   // (no dynamic index: the record stays in registers)
        if (c == ev.comp) r.dc[c] = (uint16_t)(r.dc[c] + (uint32_t)ev.value);
    }
    if (ev.block_done) ++r.blocks;
    return true;
  }
};

// Subsequence t in round `round` (1-based).  prev: the exit table the round before wrote.  -> t's entry of this round's table;
// *rec is rewritten when t decodes.
RART_JPEG_HD inline uint32_t par_round(const ParImage& I, int t, int round, const uint32_t* prev, ParRecord* rec) {
  uint32_t entry;
  if (round == 1) {
    entry = t == 0 ? par_pack(0, 0, 0) : par_guess(I, t);
  } else {
    if (t == 0 || !(prev[t - 1] & kParChanged)) return prev[t] & kParState;
    entry = prev[t - 1] & kParState;
  }
  ParCount count;
  const uint32_t ex = par_decode(I, t, entry, count);
  *rec = count.r;
  return ex | ((round == 1 || ex != (prev[t] & kParState)) ? kParChanged : 0u);
}

struct ParWrite {
  const ParImage& I;
  int16_t* coef;          // the image's coefficients, zeroed
  int B;                  // scan-order number of the block being decoded
  uint32_t pred[3];
  bool invalid = false;   // the chain met an error below the block total
  RART_JPEG_HD ParWrite(const ParImage& img, int16_t* c, const ParRecord& before) : I(img), coef(c), B((int)before.blocks) {
    for (int i = 0; i < 3; ++i) pred[i] = before.dc[i];
  }
  RART_JPEG_HD bool operator()(const ParEvent& ev) {
    if (B < 0 || B >= I.total_blocks) return false;   // what follows the last block is ignored
    if (ev.kind == kParError) {
      invalid = true;
      return false;
    }
    if (ev.kind == kParDC) {
      uint32_t p = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c == ev.comp) p = pred[c] += (uint32_t)ev.value;
      coef[par_block_addr(I, B)] = (int16_t)(uint16_t)p;
    } else if (ev.kind == kParAC && ev.k >= 1 && ev.k < 64) {
      coef[par_block_addr(I, B) + par_natural(ev.k)] = (int16_t)ev.value;
    }
    if (ev.block_done) ++B;
    return true;
  }
};

// Subsequence t of the write pass.  entry: its true entry; before: the prefix sums in front of it.  -> false: RART_ERR_INVALID.
RART_JPEG_HD inline bool par_write(const ParImage& I, int t, uint32_t entry, const ParRecord& before, int16_t* coef) {
  ParWrite wr(I, coef, before);
  par_decode(I, t, entry, wr);
  return !wr.invalid;
}

RART_JPEG_HD inline void par_add(ParRecord* a, const ParRecord& b) {
  a->blocks += b.blocks;
  for (int i = 0; i < 3; ++i) a->dc[i] = (uint16_t)(a->dc[i] + b.dc[i]);
}

// ---- host side: the plan of one file and the emulation of the device rounds ----

struct ParPlan {
  int host_path;           // 1: the sequential decoder takes this file (restart interval, scan or table count beyond the limits)
  size_t scan_pos, stop;
  int scan_len, nsub;
  int ntab, dc_tab[3], ac_tab[3];
  const Huff* tab[kParMaxTables];
};

// first marker (FF followed by anything but 00) or the end of the data, as Bits::fill sees it
inline size_t find_stop(const uint8_t* data, size_t len, size_t from) {
  size_t q = from;
  while (q < len) {
    const void* ff = memchr(data + q, 0xFF, len - q);
    if (!ff) break;
    q = (size_t)((const uint8_t*)ff - data);
    if (q + 1 >= len || data[q + 1] != 0) return q;
    q += 2;
  }
  return len;
}

inline void make_plan(const uint8_t* data, size_t len, const Parsed& P, int subseq_bytes, ParPlan* pl) {
  memset(pl, 0, sizeof(*pl));
  pl->scan_pos = P.scan_pos;
  pl->stop = find_stop(data, len, P.scan_pos);
  const size_t scan_len = pl->stop - pl->scan_pos;
  for (int c = 0; c < P.ncomp; ++c) {
    for (int cls = 0; cls < 2; ++cls) {
      const Huff* h = cls ? &P.ac[P.ta[c]] : &P.dc[P.td[c]];
      int j = 0;
      while (j < pl->ntab && pl->tab[j] != h) ++j;
      if (j == pl->ntab) {
        if (pl->ntab == kParMaxTables) {
          pl->host_path = 1;
          j = 0;
        } else {
          pl->tab[pl->ntab++] = h;
        }
      }
      (cls ? pl->ac_tab : pl->dc_tab)[c] = j;
    }
  }
  if (P.restart_interval != 0 || scan_len > (size_t)kParMaxScanBytes) pl->host_path = 1;
  const size_t nsub = (scan_len + subseq_bytes - 1) / subseq_bytes;
  if (nsub > (size_t)kParMaxSubseq) pl->host_path = 1;
  pl->scan_len = pl->host_path ? 0 : (int)scan_len;
  pl->nsub = pl->host_path ? 0 : (int)nsub;
}

inline bool par_subseq_ok(int subseq_bytes) { return subseq_bytes >= 4 && subseq_bytes <= 65536 && (subseq_bytes & (subseq_bytes - 1)) == 0; }

inline void par_image(const Parsed& P, const rart_jpeg_info& now, const ParPlan& pl, const uint8_t* scan, int subseq_bytes, ParImage* I) {
  memset(I, 0, sizeof(*I));
  I->scan = scan;
  I->scan_len = pl.scan_len;
  I->nsub = pl.nsub;
  I->subseq_bytes = subseq_bytes;
  I->ncomp = P.ncomp;
  I->hs = P.hs[0];
  I->vs = P.vs[0];
  I->nslots = P.ncomp == 1 ? 1 : P.hs[0] * P.vs[0] + 2;
  I->mcux = now.blocks_w[0] / P.hs[0];
  int start = 0;
  for (int c = 0; c < 3; ++c) {
    const int cc = c < P.ncomp ? c : 0;
    I->dc[c] = pl.tab[pl.dc_tab[cc]];
    I->ac[c] = pl.tab[pl.ac_tab[cc]];
    I->bw[c] = c < P.ncomp ? now.blocks_w[c] : 0;
    I->comp_start[c] = start;
    if (c < P.ncomp) start += now.blocks_w[c] * now.blocks_h[c];
  }
  I->total_blocks = start;
}

// The device's rounds, cap, prefix sums and write pass on the host, for one file; scratch for 2 nsub states and nsub records is
// the caller's (no allocation here).  -> status; *rounds_used: the rounds run (0 when the sequential decoder took the file).
inline Result par_emulate_image(const ParImage& I, int max_rounds, int16_t* coef, uint32_t* exits, ParRecord* recs, int* rounds_used) {
  *rounds_used = 0;
  if (I.nsub == 0) return {RART_ERR_INVALID, "empty entropy-coded segment"};
  uint32_t* tab[2] = {exits, exits + I.nsub};
  int cur = 0;
  bool converged = false;
  for (int round = 1; round <= max_rounds && !converged; ++round) {
    bool any = false;
    for (int t = 0; t < I.nsub; ++t) {
      const uint32_t v = par_round(I, t, round, tab[cur ^ 1], &recs[t]);
      tab[cur][t] = v;
      any = any || (v & kParChanged);
    }
    cur ^= 1;
    *rounds_used = round;
    converged = !any;
  }
  if (!converged) return {RART_ERR_UNSUPPORTED, "not converged within max_rounds (decode it sequentially)"};
  const uint32_t* ex = tab[cur ^ 1];
  ParRecord run = {0, {0, 0, 0}, 0};
  for (int t = 0; t < I.nsub; ++t) {
    const ParRecord own = recs[t];
    recs[t] = run;
    par_add(&run, own);
  }
  bool ok = run.blocks >= (uint32_t)I.total_blocks;
  for (int t = 0; t < I.nsub; ++t) ok = par_write(I, t, t == 0 ? par_pack(0, 0, 0) : ex[t - 1], recs[t], coef) && ok;
  return ok ? Result{RART_OK, ""} : Result{RART_ERR_INVALID, "truncated or corrupt entropy data"};
}

// rart_jpeg_entropy_emulate: entropy_decode's contract (same argument checks, same statuses, same coefficients), computed the
// device's way.  subseq_bytes / max_rounds: 0 = the defaults.
inline Result emulate(const uint8_t* data, size_t len, const rart_jpeg_info* info, int subseq_bytes, int max_rounds, int16_t* coef,
                      size_t capacity, int* rounds_used) {
  if (!info || !coef || !rounds_used) return {RART_ERR_INVALID, "null info / coef / rounds_used"};
  *rounds_used = 0;
  if (subseq_bytes == 0) subseq_bytes = kParDefaultSubseq;
  if (max_rounds == 0) max_rounds = kParDefaultRounds;
  if (!par_subseq_ok(subseq_bytes)) return {RART_ERR_INVALID, "subseq_bytes must be a power of two from 4 to 65536"};
  if (max_rounds < 0) return {RART_ERR_INVALID, "negative max_rounds"};
  Parsed P;
  const Result r = parse(data, len, &P);
  if (r.status != RART_OK) return r;
  ParPlan pl;
  make_plan(data, len, P, subseq_bytes, &pl);
  if (pl.host_path) return entropy_decode(data, len, info, coef, capacity);
  rart_jpeg_info now;
  memset(&now, 0, sizeof(now));
  fill_info(P, &now);
  if (info->status != RART_OK || now.height != info->height || now.width != info->width || now.ncomp != info->ncomp ||
      now.coef_count != info->coef_count)
    return {RART_ERR_INVALID, "info does not describe this file (probe it first)"};
  if ((uint64_t)now.coef_count > (uint64_t)capacity) return {RART_ERR_INVALID, "coefficient buffer too small"};
  memset(coef, 0, (size_t)now.coef_count * sizeof(int16_t));
  ParImage I;
  par_image(P, now, pl, data + pl.scan_pos, subseq_bytes, &I);
  if (I.nsub == 0) return {RART_ERR_INVALID, "empty entropy-coded segment"};
  uint32_t* exits = (uint32_t*)malloc((size_t)I.nsub * 2 * sizeof(uint32_t));
  ParRecord* recs = (ParRecord*)malloc((size_t)I.nsub * sizeof(ParRecord));
  Result out = {RART_ERR_INVALID, "out of memory"};
  if (exits && recs) out = par_emulate_image(I, max_rounds, coef, exits, recs, rounds_used);
  free(exits);
  free(recs);
  return out;
}

// rart_jpeg_scan_plan's descriptor (the caller's four offsets stay as they are)
inline void fill_scan(const Parsed& P, const rart_jpeg_info& now, const ParPlan& pl, rart_jpeg_scan* s) {
  s->scan_pos = (int64_t)pl.scan_pos;
  s->scan_len = pl.scan_len;
  s->nsub = pl.nsub;
  s->host_path = pl.host_path;
  s->ntab = pl.host_path ? 0 : pl.ntab;
  s->ncomp = P.ncomp;
  s->h_samp = P.hs[0];
  s->v_samp = P.vs[0];
  s->mcux = now.blocks_w[0] / P.hs[0];
  s->mcuy = now.blocks_h[0] / P.vs[0];
  for (int c = 0; c < 3; ++c) {
    s->dc_tab[c] = c < P.ncomp && !pl.host_path ? pl.dc_tab[c] : 0;
    s->ac_tab[c] = c < P.ncomp && !pl.host_path ? pl.ac_tab[c] : 0;
    s->blocks_w[c] = c < P.ncomp ? now.blocks_w[c] : 0;
    s->blocks_h[c] = c < P.ncomp ? now.blocks_h[c] : 0;
  }
  s->reserved_ = 0;
}

}  // namespace rart_jpeg
