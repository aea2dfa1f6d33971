// Prints the tables of sf_layout.h -- groups, kFields, kBitFields and the constants beside them -- one record per line, for
// tests/test_lane_row_model.py to compare with the numpy row codec's own table (tests/lanerow_np.py).  Host only.
#include <stdio.h>

#include "sf_layout.h"

int main() {
  static const char* const group_names[] = {
#define G(name, chunk, slots) #name,
      SF_GROUPS(G)
#undef G
  };
  for (int g = 0; g < SF_G_COUNT; g++)
    printf("group %s %d %d %ld\n", group_names[g], sfl::kGroups[g].chunk, sfl::kGroups[g].slots, sfl::group_offset(g));
  for (int f = 0; f < SF_F_COUNT; f++) {
    const sfl::FieldMeta& m = sfl::kFields[f];
    printf("field %s %d %d %d %s %d %d\n", m.name, m.elem_size, m.count, m.is_float, group_names[m.group], m.byte_in_chunk, m.kind);
  }
  for (const sfl::BitField& b : sfl::kBitFields) printf("bits %s %d %d %d\n", sfl::kFields[b.field].name, b.shift, b.bits, b.is_signed);
  printf("const nslot %d\nconst nstat %d\nconst keycount_byte %d\nconst key_first %d\nconst key_count %d\n", SF_NSLOT, SF_NSTAT,
         SF_KEYCOUNT_BYTE, SF_ST_KEY_FIRST, SF_ST_KEY_COUNT);
  printf("const mask_bits %d\nconst mask_low %u\nconst mpool_shift %d\nconst kills_shift %d\n", SF_MASK_BITS, SF_MASK_LOW, SF_MPOOL_SHIFT,
         SF_KILLS_SHIFT);
  printf("const mm_angle_max %u\nconst bytes_per_lane %ld\n", SF_MM_ANGLE(~0u), sfl::kBytesPerLane);
  return 0;
}
