// Stand-alone driver of csrc/jpeg_entropy_par.h for malformed input (built with -fsanitize=address,undefined by
// tests/test_jpeg_entropy_par_cpu.py): every prefix truncation of the file named on the command line, and every single-byte
// overwrite of the first 256 bytes of its scan with 0x00 / 0xFF / 0xD0 / the byte's complement, goes through the sequential decoder
// and through the emulation of the parallel one at subseq_bytes 4 and 32.  The two statuses must be equal, and the coefficients
// whenever both are RART_OK; the sanitizers report any read or write outside the buffers.  Exit 0 = all runs agreed.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../robustart_amd/csrc/jpeg_entropy_par.h"

static long g_runs = 0, g_ok = 0, g_invalid = 0, g_other = 0, g_max_rounds = 0;

// the input lives in an exactly-sized heap block, so a read one byte past `len` is a heap-buffer-overflow
static void run(const std::vector<uint8_t>& bytes, size_t len) {
  uint8_t* data = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(data, bytes.data(), len);
  rart_jpeg_info info;
  rart_jpeg::probe(data, len, &info);
  const size_t count = info.status == RART_OK ? (size_t)info.coef_count : 64;
  std::vector<int16_t> want(count, 0), got(count, 0);
  const rart_jpeg::Result seq = rart_jpeg::entropy_decode(data, len, &info, want.data(), want.size());
  const int sizes[2] = {4, 32};
  for (int i = 0; i < 2; ++i) {
    int rounds = -1;
    const rart_jpeg::Result par = rart_jpeg::emulate(data, len, &info, sizes[i], 1 << 20, got.data(), got.size(), &rounds);
    if (par.status != seq.status) {
      fprintf(stderr, "len %zu subseq_bytes %d: sequential status %d (%s), emulation %d (%s)\n", len, sizes[i], seq.status, seq.why,
              par.status, par.why);
      exit(3);
    }
    if (seq.status == RART_OK && got != want) {
      fprintf(stderr, "len %zu subseq_bytes %d: coefficients differ\n", len, sizes[i]);
      exit(4);
    }
    if (rounds > g_max_rounds) g_max_rounds = rounds;
  }
  free(data);
  ++g_runs;
  if (seq.status == RART_OK) ++g_ok;
  else if (seq.status == RART_ERR_INVALID) ++g_invalid;
  else ++g_other;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> file;
  for (int c; (c = fgetc(f)) != EOF;) file.push_back((uint8_t)c);
  fclose(f);
  rart_jpeg::Parsed P;
  if (rart_jpeg::parse(file.data(), file.size(), &P).status != RART_OK) return 5;
  run(file, file.size());
  if (g_ok != 1) {
    fprintf(stderr, "the intact file does not decode\n");
    return 5;
  }
  for (size_t len = 0; len < file.size(); ++len) run(file, len);
  const size_t span = P.scan_pos + 256 < file.size() ? P.scan_pos + 256 : file.size();
  for (size_t i = P.scan_pos; i < span; ++i) {
    const uint8_t subst[4] = {0x00, 0xFF, 0xD0, (uint8_t)~file[i]};
    for (int k = 0; k < 4; ++k) {
      std::vector<uint8_t> m = file;
      m[i] = subst[k];
      run(m, m.size());
    }
  }
  printf("runs %ld ok %ld invalid %ld other %ld max_rounds %ld\n", g_runs, g_ok, g_invalid, g_other, g_max_rounds);
  return 0;
}
