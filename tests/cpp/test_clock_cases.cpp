// fh::clock_loop and fh::clock_at (faster_amd/csrc/fh_clock.hpp) on cases given by the caller, printed bit for bit: the Python model of
// the sample clock (tests/sample_model.py) is compared with both by tests/test_sample_model.py.
//   input  (stdin):  one case per line: <DC bits, hex> <dt bits, hex> <N> <n samples>
//   output (stdout): per case and sample k = 0 .. n - 1: <t of the loop, hex bits> <interval> <t of clock_at, hex bits> <interval>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../faster_amd/csrc/fh_clock.hpp"

static double from_bits(unsigned long long b) {
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
static unsigned long long to_bits(double d) {
  unsigned long long b;
  std::memcpy(&b, &d, 8);
  return b;
}

int main() {
  unsigned long long dcb, dtb;
  int N, n;
  while (std::scanf("%llx %llx %d %d", &dcb, &dtb, &N, &n) == 4) {
    const double DC = from_bits(dcb), dt = from_bits(dtb);
    for (int k = 0; k < n; k++) {
      double t0, t1;
      int i0, i1;
      fh::clock_loop(k, DC, dt, N, t0, i0);
      fh::clock_at(k, DC, dt, N, t1, i1);
      std::printf("%llx %d %llx %d\n", to_bits(t0), i0, to_bits(t1), i1);
    }
  }
  return 0;
}
