// Host program of tests/test_sort_elem_host.py: the packed sort_temp element of csrc/common.hpp (sort_pack / sort_sub /
// sort_idx_sign, range_first_key) and the dispatch rule sort_elem_bytes, compiled for the host alone.
//   sort_elem_host pack IDX SIGN SUB      ->  "V SUB' IDX_SIGN'"  (the packed word, then what unpacks from it)
//   sort_elem_host bytes COLUMNS WIDE     ->  "4" or "8"
//   sort_elem_host first RANGE SHIFT      ->  first key of the range
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.hpp"

int main(int argc, char** argv) {
  using namespace msm377;
  if (argc == 5 && !strcmp(argv[1], "pack")) {
    const SortElem4 e = sort_pack((uint32_t)strtoul(argv[2], nullptr, 0), (uint32_t)strtoul(argv[3], nullptr, 0), (uint32_t)strtoul(argv[4], nullptr, 0));
    static_assert(sizeof(SortElem4) == 4 && sizeof(SortElem) == 8, "element sizes");
    printf("%u %u %u\n", e.v, sort_sub(e), sort_idx_sign(e));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "bytes")) {
    printf("%u\n", sort_elem_bytes(strtoull(argv[2], nullptr, 0), atoi(argv[3]) != 0));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "first")) {
    printf("%u\n", range_first_key((uint32_t)strtoul(argv[2], nullptr, 0), (uint32_t)strtoul(argv[3], nullptr, 0)));
    return 0;
  }
  fprintf(stderr, "usage: sort_elem_host pack IDX SIGN SUB | bytes COLUMNS WIDE | first RANGE SHIFT\n");
  return 2;
}
