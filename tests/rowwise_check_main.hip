// Stand-alone host program: the operand check of csrc/kernels/rowwise.h, called directly.  It
// touches no device and makes no HIP call; test_rowwise_check.py builds it with the host side
// under AddressSanitizer / UBSan and runs it.  Exit status: the number of failed expectations.
#include <cstdio>

#include "kernels/rowwise.h"

using namespace nnmpi;

static int failed = 0;

static void expect(const char* what, hipError_t got, hipError_t want, int vec, int want_vec) {
  if (got == want && vec == want_vec) return;
  std::printf("FAIL %s: error %d (want %d), width %d (want %d)\n", what, (int)got, (int)want, vec,
              want_vec);
  ++failed;
}

int main() {
  const hipError_t OK = hipSuccess, BAD = hipErrorInvalidValue;
  // 16-byte aligned backing store, never dereferenced by the check
  alignas(16) static char buf[1 << 16];
  char* a = buf;
  char* b = buf + (1 << 15);
  int aux = 0, v = -1;
#define CHECK(what, want, want_vec, ...) \
  v = -1;                                \
  expect(what, row_check(__VA_ARGS__, &v), want, v, want_vec)
  //                     bf16 p0 ld0  p1 ld1  aux  rows H  op_ok
  CHECK("no rows, null pointers", OK, 0, 0, nullptr, 16, nullptr, 16, nullptr, 0, 16, true);
  CHECK("no rows, op arguments invalid", BAD, 0, 0, nullptr, 16, nullptr, 16, nullptr, 0, 16, false);
  CHECK("no rows, H = 0", BAD, 0, 0, nullptr, 16, nullptr, 16, nullptr, 0, 0, true);
  CHECK("negative rows", BAD, 0, 0, a, 16, b, 16, &aux, -1, 16, true);
  CHECK("null operand", BAD, 0, 0, a, 16, nullptr, 16, &aux, 1, 16, true);
  CHECK("null third operand", BAD, 0, 0, a, 16, b, 16, nullptr, 1, 16, true);
  CHECK("one row, ld < H", BAD, 0, 0, a, 8, b, 16, &aux, 1, 16, true);
  CHECK("one row, ld == H", OK, 4, 0, a, 16, b, 16, &aux, 1, 16, true);
  CHECK("H = 8192 fp32", OK, 4, 0, a, 8192, b, 8192, &aux, 1, 8192, true);
  CHECK("H = 8192 bf16", OK, 8, 1, a, 8192, b, 8192, &aux, 1, 8192, true);
  CHECK("H = 8200", BAD, 0, 0, a, 8200, b, 8200, &aux, 1, 8200, true);
  CHECK("bf16 H = 12", BAD, 0, 1, a, 16, b, 16, &aux, 2, 12, true);
  CHECK("bf16 H = 16, stride 20", BAD, 0, 1, a, 20, b, 16, &aux, 2, 16, true);
  CHECK("bf16 H = 16", OK, 8, 1, a, 16, b, 24, &aux, 2, 16, true);
  CHECK("fp32 H = 3", OK, 1, 0, a, 3, b, 3, &aux, 5, 3, true);
  CHECK("fp32 H = 8, stride 10", OK, 1, 0, a, 10, b, 8, &aux, 5, 8, true);
  CHECK("fp32 misaligned base", OK, 1, 0, a + 4, 8, b, 8, &aux, 5, 8, true);
  CHECK("bf16 misaligned base", BAD, 0, 1, a + 2, 8, b, 8, &aux, 5, 8, true);
  // two operands one row apart: two rows overlap, one row does not
  CHECK("overlap one row apart, fp32", BAD, 0, 0, a, 8, a + 8 * 4, 8, &aux, 2, 8, true);
  CHECK("overlap one row apart, bf16", BAD, 0, 1, a, 8, a + 8 * 2, 8, &aux, 2, 8, true);
  CHECK("one row apart, one row", OK, 4, 0, a, 8, a + 8 * 4, 8, &aux, 1, 8, true);
  CHECK("same operand", BAD, 0, 0, a, 8, a, 8, &aux, 1, 8, true);
  // interleaved columns of one buffer count as overlapping (byte ranges, not elements)
  CHECK("interleaved columns", BAD, 0, 0, a, 16, a + 8 * 4, 16, &aux, 2, 8, true);
  if (!act_known(ACT_NONE) || !act_known(ACT_RELU) || !act_known(ACT_TANH) || act_known(3) ||
      act_known(-1)) {
    std::printf("FAIL act_known\n");
    ++failed;
  }
  std::printf("%s\n", failed ? "rowwise check: FAILED" : "rowwise check: ok");
  return failed;
}
