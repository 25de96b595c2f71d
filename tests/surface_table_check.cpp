// Prints the marching-tetrahedra tables of csrc/surface_table.h, host only: six rows of tet
// corner codes, then the 6 x 16 case rows.  tests/test_surface_cpu.py compares the text with the
// restatement's own derivation.
#include <cstdint>
#include <cstdio>

#include "surface_table.h"

static const uint8_t kCorners[6][4] = RS_SURFACE_TET_CORNERS;
static const uint8_t kTable[6][16][7] = RS_SURFACE_TET_TABLE;

int main() {
  for (int k = 0; k < 6; ++k)
    std::printf("%d %d %d %d\n", kCorners[k][0], kCorners[k][1], kCorners[k][2], kCorners[k][3]);
  for (int k = 0; k < 6; ++k)
    for (int c = 0; c < 16; ++c) {
      for (int j = 0; j < 7; ++j) std::printf(j ? " %d" : "%d", kTable[k][c][j]);
      std::printf("\n");
    }
  return 0;
}
