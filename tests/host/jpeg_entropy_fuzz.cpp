// Stand-alone driver of csrc/jpeg_entropy.h for malformed input (built with -fsanitize=address,undefined by
// tests/test_jpeg_reader_cpu.py): every prefix truncation of the file named on the command line, and every single-byte overwrite
// with 0x00 / 0xFF / 0x7F over its header and the first 256 bytes of its scan, goes through probe + entropy decode.  Each run must
// return a status; the sanitizers report any read or write outside the buffers.  Exit 0 = all runs returned.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../robustart_amd/csrc/jpeg_entropy.h"

static long g_runs = 0, g_ok = 0, g_unsupported = 0, g_invalid = 0;

// the input lives in an exactly-sized heap block, so a read one byte past `len` is a heap-buffer-overflow
static int run(const std::vector<uint8_t>& bytes, size_t len) {
  uint8_t* data = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(data, bytes.data(), len);
  rart_jpeg_info info;
  rart_jpeg::Result r = rart_jpeg::probe(data, len, &info);
  if (r.status == RART_OK) {
    std::vector<int16_t> coef((size_t)info.coef_count);
    r = rart_jpeg::entropy_decode(data, len, &info, coef.data(), coef.size());
    if (info.coef_count > 0) {
      const rart_jpeg::Result small = rart_jpeg::entropy_decode(data, len, &info, coef.data(), coef.size() - 1);
      if (small.status != RART_ERR_INVALID) {
        fprintf(stderr, "a coefficient buffer one element short was accepted\n");
        exit(3);
      }
    }
  }
  free(data);
  ++g_runs;
  if (r.status == RART_OK) ++g_ok;
  else if (r.status == RART_ERR_UNSUPPORTED) ++g_unsupported;
  else if (r.status == RART_ERR_INVALID) ++g_invalid;
  else {
    fprintf(stderr, "unexpected status %d\n", r.status);
    exit(4);
  }
  return r.status;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> file;
  for (int c; (c = fgetc(f)) != EOF;) file.push_back((uint8_t)c);
  fclose(f);
  if (run(file, file.size()) != RART_OK) {
    fprintf(stderr, "the intact file does not decode\n");
    return 5;
  }
  rart_jpeg::Parsed P;
  if (rart_jpeg::parse(file.data(), file.size(), &P).status != RART_OK) return 5;
  for (size_t len = 0; len < file.size(); ++len) {
    if (run(file, len) == RART_OK && len + 2 < file.size()) {   // only the two bytes of the EOI marker may go missing
      fprintf(stderr, "the prefix of %zu bytes decoded as if it were complete\n", len);
      return 6;
    }
  }
  const size_t span = P.scan_pos + 256 < file.size() ? P.scan_pos + 256 : file.size();
  const uint8_t subst[3] = {0x00, 0xFF, 0x7F};
  for (size_t i = 0; i < span; ++i) {
    for (int k = 0; k < 3; ++k) {
      std::vector<uint8_t> m = file;
      m[i] = subst[k];
      run(m, m.size());
    }
  }
  printf("runs %ld ok %ld unsupported %ld invalid %ld\n", g_runs, g_ok, g_unsupported, g_invalid);
  return 0;
}
