/* ORACLE — TEST INFRASTRUCTURE ONLY (see zo_common.h). Stand-alone sanitizer check of the restated decoder on crafted frames:
   `make -C oracle craft-check` builds this file and the oracle's sources with -fsanitize=address,undefined, lets tests/frame_craft.py
   write its randomised frames (fixed seeds) and its directed frames into a file, and decodes every one of them with zo_decompress.
   Record: u32 frame bytes, u32 plaintext bytes, u32 expected zstd error code (0: decodes), u64 XXH64 of the plaintext, the frame.
   Host only: not a pytest test, not loaded into Python. */
#include <stdio.h>
#include <stdlib.h>
#include "zo_internal.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s frames.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  unsigned n = 0, bad = 0;
  u8 head[20];
  while (fread(head, 1, 20, f) == 20) {
    const u32 fl = rd32(head), pl = rd32(head + 4), code = rd32(head + 8);
    const u64 want = rd64(head + 12);
    /* exact-size buffers, so that a read or write one byte beyond either is reported */
    u8* src = (u8*)malloc(fl ? fl : 1);
    u8* dst = (u8*)malloc(pl ? pl : 1);
    if (!src || !dst || fread(src, 1, fl, f) != fl) { fprintf(stderr, "frame %u: short file\n", n); return 2; }
    const size_t r = zo_decompress(dst, pl, src, fl);
    if (code) {
      if (!ZO_ISERR(r) || (u32)ZO_ERRCODE(r) != code) { fprintf(stderr, "frame %u: status %d, expected %u\n", n, ZO_ISERR(r) ? ZO_ERRCODE(r) : 0, code); bad++; }
    } else if (r != pl || zo_xxh64(dst, pl, 0) != want) {
      fprintf(stderr, "frame %u: %zu bytes (error %d), expected %u\n", n, r, ZO_ISERR(r) ? ZO_ERRCODE(r) : 0, pl); bad++;
    }
    free(src); free(dst);
    n++;
  }
  fclose(f);
  printf("craft-check: %u frames, %u bad\n", n, bad);
  return bad || !n ? 1 : 0;
}
