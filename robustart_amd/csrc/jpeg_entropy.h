// Host half of the JPEG reader: marker parsing and Huffman (entropy) decoding of baseline files, plain C++17, no HIP.
// The device half (csrc/jpeg_decode.hip) takes the coefficients this produces through dequantise + IDCT + upsampling + colour
// conversion; together they reproduce Pillow's Image.open(f).convert('RGB') bit for bit.
//
// Supported set: SOF0, 8-bit samples, 8-bit quantisation tables, one scan; one component, or three with chroma (1,1) and luma
// (1,1) / (2,1) / (2,2) that libjpeg reads as YCbCr (a JFIF APP0, or an Adobe APP14 with transform 1, or no Adobe marker and
// component ids 1, 2, 3).  Everything else is RART_ERR_UNSUPPORTED (the caller decodes it with Pillow); a supported file whose
// stream is truncated or corrupt is RART_ERR_INVALID -- never padded or guessed.
//
// The input is untrusted file bytes: every read is bounded by `len`, table ids, code lengths, symbol categories and the
// coefficient index are range-checked, nothing throws, allocates or exits.  All state is local: any number of threads may decode
// different files at once.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/robustart_hip.h"

// what the device half of the parallel entropy decoder (csrc/jpeg_entropy_par.h, csrc/jpeg_entropy_gpu.hip) compiles too
#if defined(__HIPCC__)
#define RART_JPEG_HD __host__ __device__
#else
#define RART_JPEG_HD
#endif

namespace rart_jpeg {

constexpr int64_t kMaxPixels = (int64_t)1 << 26;   // larger frames are left to Pillow (and its decompression-bomb check)

static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool defined = false;
  int nvals = 0;
  uint8_t vals[256];
  int32_t mincode[17], maxcode[17], valptr[17];   // per code length 1..16; maxcode -1 = no code of that length
  uint8_t fast_len[512], fast_sym[512];           // 9-bit lookahead: code length (0 = longer than 9 bits) and symbol
};

struct Parsed {
  int height = 0, width = 0, ncomp = 0;
  int comp_id[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0};
  int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  bool qt_defined[4] = {false, false, false, false};
  uint16_t qt[4][64];       // natural order
  Huff dc[4], ac[4];
  int restart_interval = 0;
  size_t scan_pos = 0;      // first byte of the entropy-coded segment
};

struct Result {
  int status;
  const char* why;
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// DHT payload of one table: 16 counts, then the symbols.  Returns the bytes consumed, 0 on a malformed table.
inline size_t read_huff(const uint8_t* p, size_t avail, Huff* h) {
  if (avail < 16) return 0;
  int total = 0, code = 0;
  int count[17];
  for (int l = 1; l <= 16; ++l) {
    count[l] = p[l - 1];
    total += count[l];
    code += count[l];
    if (code > (1 << l)) return 0;   // more codes than the length has room for
    code <<= 1;
  }
  if (total > 256 || avail < (size_t)16 + total) return 0;
  h->nvals = total;
  memcpy(h->vals, p + 16, total);
  memset(h->fast_len, 0, sizeof(h->fast_len));
  memset(h->fast_sym, 0, sizeof(h->fast_sym));
  code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    h->valptr[l] = k;
    h->mincode[l] = code;
    if (l <= 9) {
      for (int i = 0; i < count[l]; ++i) {
        const int first = (code + i) << (9 - l);
        for (int f = 0; f < (1 << (9 - l)); ++f) {
          h->fast_len[first + f] = (uint8_t)l;
          h->fast_sym[first + f] = h->vals[k + i];
        }
      }
    }
    k += count[l];
    code += count[l];
    h->maxcode[l] = count[l] ? code - 1 : -1;
    code <<= 1;
  }
  h->defined = true;
  return (size_t)16 + total;
}

// Walks the markers up to and including the first SOS.
inline Result parse(const uint8_t* data, size_t len, Parsed* P) {
  if (!data || len < 4 || data[0] != 0xFF || data[1] != 0xD8) return {RART_ERR_UNSUPPORTED, "not a JPEG file (no SOI)"};
  size_t pos = 2;
  bool jfif = false, adobe = false, sof = false;
  int adobe_transform = 0;
  for (;;) {
    if (pos >= len) return {RART_ERR_INVALID, "truncated before the scan"};
    if (data[pos] != 0xFF) return {RART_ERR_INVALID, "marker expected"};
    while (pos < len && data[pos] == 0xFF) ++pos;   // fill bytes
    if (pos >= len) return {RART_ERR_INVALID, "truncated in a marker"};
    const int m = data[pos++];
    if (m == 0xD9) return {RART_ERR_INVALID, "EOI before any scan"};
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return {RART_ERR_INVALID, "stand-alone marker in the header"};
    if (pos + 2 > len) return {RART_ERR_INVALID, "truncated segment length"};
    const size_t seg = (size_t)be16(data + pos);
    if (seg < 2 || pos + seg > len) return {RART_ERR_INVALID, "segment runs past the end of the file"};
    const uint8_t* p = data + pos + 2;
    const size_t n = seg - 2;
    switch (m) {
      case 0xC0: {
        if (sof) return {RART_ERR_INVALID, "second frame header"};
        if (n < 6) return {RART_ERR_INVALID, "short SOF0"};
        if (p[0] != 8) return {RART_ERR_UNSUPPORTED, "sample precision is not 8 bits"};
        P->height = be16(p + 1);
        P->width = be16(p + 3);
        const int nc = p[5];
        if (nc != 1 && nc != 3) return {RART_ERR_UNSUPPORTED, "component count is not 1 or 3"};
        if (n != (size_t)6 + 3 * nc) return {RART_ERR_INVALID, "SOF0 length does not match its component count"};
        if (P->height == 0) return {RART_ERR_UNSUPPORTED, "height deferred to a DNL segment"};
        if (P->width == 0) return {RART_ERR_INVALID, "zero width"};
        if ((int64_t)P->height * P->width > kMaxPixels) return {RART_ERR_UNSUPPORTED, "frame larger than 2^26 pixels"};
        P->ncomp = nc;
        for (int c = 0; c < nc; ++c) {
          P->comp_id[c] = p[6 + 3 * c];
          P->hs[c] = p[7 + 3 * c] >> 4;
          P->vs[c] = p[7 + 3 * c] & 15;
          P->tq[c] = p[8 + 3 * c];
          if (P->hs[c] < 1 || P->hs[c] > 4 || P->vs[c] < 1 || P->vs[c] > 4) return {RART_ERR_INVALID, "sampling factor outside 1..4"};
          if (P->tq[c] > 3) return {RART_ERR_INVALID, "quantisation table id outside 0..3"};
        }
        if (nc == 1) {
          P->hs[0] = P->vs[0] = 1;   // a single-component scan is never interleaved: one block per MCU whatever the factors say
        } else {
          const bool luma_ok = (P->hs[0] == 1 && P->vs[0] == 1) || (P->hs[0] == 2 && P->vs[0] == 1) || (P->hs[0] == 2 && P->vs[0] == 2);
          if (!luma_ok || P->hs[1] != 1 || P->vs[1] != 1 || P->hs[2] != 1 || P->vs[2] != 1)
            return {RART_ERR_UNSUPPORTED, "chroma sampling other than 4:4:4, 4:2:2, 4:2:0"};
        }
        sof = true;
        break;
      }
      case 0xC1: case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC8: case 0xC9: case 0xCA: case 0xCB: case 0xCD:
      case 0xCE: case 0xCF:
        return {RART_ERR_UNSUPPORTED, "not a baseline (SOF0) frame"};
      case 0xCC:
        return {RART_ERR_UNSUPPORTED, "arithmetic coding"};
      case 0xDC:
        return {RART_ERR_UNSUPPORTED, "DNL segment"};
      case 0xC4: {
        size_t o = 0;
        while (o < n) {
          const int tc = p[o] >> 4, th = p[o] & 15;
          if (tc > 1 || th > 3) return {RART_ERR_INVALID, "Huffman table class / id out of range"};
          const size_t used = read_huff(p + o + 1, n - o - 1, tc ? &P->ac[th] : &P->dc[th]);
          if (!used) return {RART_ERR_INVALID, "malformed Huffman table"};
          o += 1 + used;
        }
        break;
      }
      case 0xDB: {
        size_t o = 0;
        while (o < n) {
          const int pq = p[o] >> 4, id = p[o] & 15;
          if (id > 3 || pq > 1) return {RART_ERR_INVALID, "quantisation table id / precision out of range"};
          if (pq == 1) return {RART_ERR_UNSUPPORTED, "16-bit quantisation table"};
          if (n - o < 65) return {RART_ERR_INVALID, "short quantisation table"};
          for (int i = 0; i < 64; ++i) P->qt[id][kNatural[i]] = p[o + 1 + i];
          P->qt_defined[id] = true;
          o += 65;
        }
        break;
      }
      case 0xDD:
        if (n != 2) return {RART_ERR_INVALID, "DRI length"};
        P->restart_interval = be16(p);
        break;
      case 0xE0:
        if (n >= 5 && memcmp(p, "JFIF\0", 5) == 0) jfif = true;
        break;
      case 0xEE:
        if (n >= 12 && memcmp(p, "Adobe", 5) == 0) {
          adobe = true;
          adobe_transform = p[11];
        }
        break;
      case 0xDA: {
        if (!sof) return {RART_ERR_INVALID, "scan before the frame header"};
        if (n < 1) return {RART_ERR_INVALID, "short SOS"};
        const int ns = p[0];
        if (ns < 1 || ns > 4 || n != (size_t)4 + 2 * ns) return {RART_ERR_INVALID, "SOS length does not match its component count"};
        if (ns != P->ncomp) return {RART_ERR_UNSUPPORTED, "more than one scan (non-interleaved components)"};
        for (int c = 0; c < ns; ++c) {
          if (p[1 + 2 * c] != P->comp_id[c]) return {RART_ERR_UNSUPPORTED, "scan components out of frame order"};
          P->td[c] = p[2 + 2 * c] >> 4;
          P->ta[c] = p[2 + 2 * c] & 15;
          if (P->td[c] > 3 || P->ta[c] > 3) return {RART_ERR_INVALID, "Huffman table id outside 0..3"};
          if (!P->dc[P->td[c]].defined || !P->ac[P->ta[c]].defined) return {RART_ERR_INVALID, "scan names an undefined Huffman table"};
          if (!P->qt_defined[P->tq[c]]) return {RART_ERR_INVALID, "frame names an undefined quantisation table"};
        }
        const uint8_t* t = p + 1 + 2 * ns;
        if (t[0] != 0 || t[1] != 63 || t[2] != 0) return {RART_ERR_UNSUPPORTED, "spectral selection / successive approximation"};
        if (P->ncomp == 3) {
          const bool ids123 = P->comp_id[0] == 1 && P->comp_id[1] == 2 && P->comp_id[2] == 3;
          if (!(jfif || (adobe && adobe_transform == 1) || (!adobe && ids123)))
            return {RART_ERR_UNSUPPORTED, "three components that are not known to be YCbCr"};
        }
        P->scan_pos = pos + seg;
        return {RART_OK, ""};
      }
      default:
        break;   // APPn, COM and the rest: skipped by length
    }
    pos += seg;
  }
}

inline void grid(const Parsed& P, int c, int* bw, int* bh) {
  const int hmax = P.hs[0], vmax = P.vs[0];   // chroma is (1,1) in the supported set, so luma carries the maxima
  const int mcux = (P.width + 8 * hmax - 1) / (8 * hmax), mcuy = (P.height + 8 * vmax - 1) / (8 * vmax);
  *bw = mcux * P.hs[c];
  *bh = mcuy * P.vs[c];
}

inline void fill_info(const Parsed& P, rart_jpeg_info* info) {
  info->height = P.height;
  info->width = P.width;
  info->ncomp = P.ncomp;
  int64_t total = 0;
  for (int c = 0; c < P.ncomp; ++c) {
    info->h_samp[c] = P.hs[c];
    info->v_samp[c] = P.vs[c];
    grid(P, c, &info->blocks_w[c], &info->blocks_h[c]);
    memcpy(info->qt[c], P.qt[P.tq[c]], sizeof(info->qt[c]));
    total += (int64_t)info->blocks_w[c] * info->blocks_h[c] * 64;
  }
  info->coef_count = total;
}

inline Result probe(const uint8_t* data, size_t len, rart_jpeg_info* info) {
  if (!info) return {RART_ERR_INVALID, "null info"};
  memset(info, 0, sizeof(*info));
  Parsed P;
  const Result r = parse(data, len, &P);
  info->status = r.status;
  if (r.status == RART_OK) fill_info(P, info);
  return r;
}

// The code at the head of `look` (16 bits, zero-padded past the end of the data) -> its length 1..16 and symbol; 0 = no code of
// the table starts these bits.
RART_JPEG_HD inline int huff_lookup(const Huff& h, uint32_t look, int* sym) {
  int l = h.fast_len[look >> 7];
  if (l) {
    *sym = h.fast_sym[look >> 7];
    return l;
  }
  for (l = 10; l <= 16; ++l) {
    const int32_t code = (int32_t)(look >> (16 - l));
    if (h.maxcode[l] >= 0 && code <= h.maxcode[l]) {
      const int idx = h.valptr[l] + code - h.mincode[l];
      if (idx < 0 || idx >= h.nvals || idx >= 256) return 0;
      *sym = h.vals[idx];
      return l;
    }
  }
  return 0;
}

// The bit reader of one entropy-coded segment.  `acc` holds the next bits left-aligned; bits past `nbits` are zero.  It stops
// feeding at a marker (FF followed by anything but 00) and at the end of the data: asking for more bits than remain is an error.
struct Bits {
  const uint8_t* p;
  size_t pos, end;
  uint64_t acc = 0;
  int nbits = 0;
  bool stopped = false;

  void fill() {
    while (nbits <= 56 && !stopped) {
      if (pos >= end) {
        stopped = true;
        break;
      }
      const uint8_t b = p[pos];
      if (b == 0xFF) {
        if (pos + 1 >= end || p[pos + 1] != 0) {
          stopped = true;
          break;
        }
        pos += 2;   // FF00 stuffing
      } else {
        ++pos;
      }
      acc |= (uint64_t)b << (56 - nbits);
      nbits += 8;
    }
  }
  bool take(int n, uint32_t* v) {   // n in 0..16
    if (n == 0) {
      *v = 0;
      return true;
    }
    if (nbits < n) fill();
    if (nbits < n) return false;
    *v = (uint32_t)(acc >> (64 - n));
    acc <<= n;
    nbits -= n;
    return true;
  }
  bool symbol(const Huff& h, int* sym) {
    if (nbits < 16) fill();
    const uint32_t look = (uint32_t)(acc >> 48);   // 16 bits, zero-padded past the end
    const int l = huff_lookup(h, look, sym);
    if (!l) return false;
    if (nbits < l) return false;
    acc <<= l;
    nbits -= l;
    return true;
  }
};

RART_JPEG_HD inline int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

inline Result entropy_decode(const uint8_t* data, size_t len, const rart_jpeg_info* info, int16_t* coef, size_t capacity) {
  if (!info || !coef) return {RART_ERR_INVALID, "null info / coef"};
  Parsed P;
  const Result r = parse(data, len, &P);
  if (r.status != RART_OK) return r;
  rart_jpeg_info now;
  memset(&now, 0, sizeof(now));
  fill_info(P, &now);
  if (info->status != RART_OK || now.height != info->height || now.width != info->width || now.ncomp != info->ncomp ||
      now.coef_count != info->coef_count)
    return {RART_ERR_INVALID, "info does not describe this file (probe it first)"};
  if ((uint64_t)now.coef_count > (uint64_t)capacity) return {RART_ERR_INVALID, "coefficient buffer too small"};
  memset(coef, 0, (size_t)now.coef_count * sizeof(int16_t));
  int16_t* plane[3];
  int bw[3], bh[3];
  {
    int16_t* q = coef;
    for (int c = 0; c < P.ncomp; ++c) {
      plane[c] = q;
      bw[c] = now.blocks_w[c];
      bh[c] = now.blocks_h[c];
      q += (size_t)bw[c] * bh[c] * 64;
    }
  }
  const int mcux = bw[0] / P.hs[0], mcuy = bh[0] / P.vs[0];
  Bits B{data, P.scan_pos, len};
  uint32_t pred[3] = {0, 0, 0};
  int until_restart = P.restart_interval, next_rst = 0;
  for (int my = 0; my < mcuy; ++my) {
    for (int mx = 0; mx < mcux; ++mx) {
      if (P.restart_interval && until_restart == 0) {
        // discard the padding bits; the reader must be standing on the marker
        B.fill();
        if (!B.stopped || B.nbits >= 8) return {RART_ERR_INVALID, "entropy data runs past a restart interval"};
        size_t q = B.pos;
        while (q < len && data[q] == 0xFF) ++q;
        if (q == B.pos || q >= len || data[q] != 0xD0 + next_rst) return {RART_ERR_INVALID, "restart marker missing or out of order"};
        B = Bits{data, q + 1, len};
        next_rst = (next_rst + 1) & 7;
        until_restart = P.restart_interval;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < P.ncomp; ++c) {
        const Huff& hd = P.dc[P.td[c]];
        const Huff& ha = P.ac[P.ta[c]];
        for (int v = 0; v < P.vs[c]; ++v) {
          for (int h = 0; h < P.hs[c]; ++h) {
            int16_t* blk = plane[c] + ((size_t)(my * P.vs[c] + v) * bw[c] + (size_t)(mx * P.hs[c] + h)) * 64;
            int s;
            uint32_t bits;
            if (!B.symbol(hd, &s)) return {RART_ERR_INVALID, "truncated or corrupt entropy data (DC code)"};
            if (s > 11) return {RART_ERR_INVALID, "DC category above 11"};
            if (s) {
              if (!B.take(s, &bits)) return {RART_ERR_INVALID, "truncated entropy data (DC bits)"};
              pred[c] += (uint32_t)extend(bits, s);
            }
            blk[0] = (int16_t)(uint16_t)pred[c];
            for (int k = 1; k < 64; ++k) {
              if (!B.symbol(ha, &s)) return {RART_ERR_INVALID, "truncated or corrupt entropy data (AC code)"};
              const int run = s >> 4;
              s &= 15;
              if (s == 0) {
                if (run != 15) break;   // end of block
                k += 15;                // ZRL
                continue;
              }
              if (s > 10) return {RART_ERR_INVALID, "AC category above 10"};
              k += run;
              if (k > 63) return {RART_ERR_INVALID, "coefficient index past 63"};
              if (!B.take(s, &bits)) return {RART_ERR_INVALID, "truncated entropy data (AC bits)"};
              blk[kNatural[k]] = (int16_t)extend(bits, s);
            }
          }
        }
      }
      if (P.restart_interval) --until_restart;
    }
  }
  return {RART_OK, ""};
}

}  // namespace rart_jpeg
