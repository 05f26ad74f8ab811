// The launch policy of the solve kernels (faster_amd/csrc/fh_policy.hpp) on the CPU: the table of regimes, the automatic choices of each,
// every explicit fh_sched field against its automatic value, and how the number of hardware queues is read.  Prints "ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../faster_amd/csrc/fh_policy.hpp"

static int checks = 0, failed = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    checks++;                                                     \
    if (!(c)) {                                                   \
      failed++;                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
    }                                                             \
  } while (0)

static fh_sched defaults() {  // what fh_default_sched sets in the fields the policy reads
  fh_sched s;
  std::memset(&s, 0, sizeof(s));
  s.launch_order = 1;
  s.publish_factor = 4;
  s.backlog = 32;
  s.min_nodes = 2;
  return s;
}

int main() {
  using namespace fhp;
  const int CU = 256, BIG = 32768;
  const fh_sched d = defaults();

  // the table of regimes: others 0, 1, 3, 4, 13 against queues 1, 4, 16
  const int others[5] = {0, 1, 3, 4, 13}, queues[3] = {1, 4, 16};
  const Regime want[5][3] = {{ALONE, ALONE, ALONE},
                             {QUEUED, BESIDE_OTHERS, BESIDE_OTHERS},
                             {QUEUED, BESIDE_OTHERS, BESIDE_OTHERS},  // 3 others + this launch == 4 queues: the last one that has a queue
                             {QUEUED, QUEUED, BESIDE_OTHERS},         // 4 others + this launch  > 4 queues
                             {QUEUED, QUEUED, BESIDE_OTHERS}};
  for (int i = 0; i < 5; i++)
    for (int j = 0; j < 3; j++) {
      CHECK(regime_of(others[i], queues[j]) == want[i][j]);
      const LaunchPolicy p = launch_policy(BIG, CU, others[i], queues[j], d);
      CHECK(p.regime == want[i][j]);
      // alone and beside others: the choices of before this header existed, exactly
      if (want[i][j] == ALONE) CHECK(p.look_every == 8 && p.sort && p.waiting_workgroups == 4);
      if (want[i][j] == BESIDE_OTHERS) CHECK(p.look_every == 16 && !p.sort && p.waiting_workgroups == 4);
      if (want[i][j] == QUEUED)
        CHECK(p.look_every == LOOK_EVERY_QUEUED && p.sort == ORDER_WHEN_QUEUED && p.waiting_workgroups == CU / WAITING_CU_DIVISOR_QUEUED);
      CHECK(p.publish_factor == 4 && p.backlog == 32);
      CHECK(p.look_every >= 2 && p.look_every <= 1024 && (p.look_every & (p.look_every - 1)) == 0 && p.waiting_workgroups >= 2);
    }
  // the boundary others + 1 == queues from both sides, for every queue count the library believes
  for (int q = 1; q <= QUEUES_MAX; q++) {
    CHECK(regime_of(q, q) == QUEUED);
    CHECK(regime_of(q - 1, q) == (q == 1 ? ALONE : BESIDE_OTHERS));
    if (q > 2) CHECK(regime_of(q - 2, q) == BESIDE_OTHERS);
  }
  CHECK(regime_of(-1, 4) == ALONE);

  // no order below 2048 units, whatever the regime and whatever the caller asks for
  fh_sched always = d;
  always.launch_order = 2;
  fh_sched never = d;
  never.launch_order = 0;
  for (int i = 0; i < 5; i++) {
    CHECK(!launch_policy(2047, CU, others[i], 4, d).sort && !launch_policy(2047, CU, others[i], 4, always).sort);
    CHECK(launch_policy(2048, CU, others[i], 4, always).sort && launch_policy(BIG, CU, others[i], 4, always).sort);
    CHECK(!launch_policy(2048, CU, others[i], 4, never).sort && !launch_policy(BIG, CU, others[i], 4, never).sort);
  }
  CHECK(launch_policy(2048, CU, 0, 4, d).sort && !launch_policy(2048, CU, 1, 4, d).sort);
  CHECK(launch_policy(2048, CU, 4, 4, d).sort == ORDER_WHEN_QUEUED);

  // small batches (up to 8 units per CU) keep CUs / 16 waiting workgroups, at least 8, in every regime
  for (int i = 0; i < 5; i++) {
    CHECK(launch_policy(8 * CU, CU, others[i], 4, d).waiting_workgroups == 16);
    CHECK(launch_policy(1, CU, others[i], 4, d).waiting_workgroups == 16);
    CHECK(launch_policy(8 * 64, 64, others[i], 4, d).waiting_workgroups == 8);
    const int w = launch_policy(8 * CU + 1, CU, others[i], 4, d).waiting_workgroups;
    CHECK(w == (regime_of(others[i], 4) == QUEUED ? CU / WAITING_CU_DIVISOR_QUEUED : 4));
    CHECK(launch_policy(8 * 64 + 1, 64, others[i], 4, d).waiting_workgroups >= 2);
  }
  CHECK(launch_policy(8 * 64 + 1, 64, 0, 4, d).waiting_workgroups == 2);

  // every explicit field wins over the automatic value, in every regime
  for (int i = 0; i < 5; i++)
    for (int j = 0; j < 3; j++) {
      fh_sched s = d;
      s.look_every = 64;
      s.waiting_workgroups = 7;
      s.publish_factor = 9;
      s.backlog = 5;
      LaunchPolicy p = launch_policy(BIG, CU, others[i], queues[j], s);
      CHECK(p.look_every == 64 && p.waiting_workgroups == 7 && p.publish_factor == 9 && p.backlog == 5);
      CHECK(launch_policy(8 * CU, CU, others[i], queues[j], s).waiting_workgroups == 7);
      s.publish_factor = 0;  // (0 is a value here: never publish ahead)
      s.backlog = 0;
      p = launch_policy(BIG, CU, others[i], queues[j], s);
      CHECK(p.publish_factor == 0 && p.backlog == 0);
      CHECK(launch_policy(BIG, CU, others[i], queues[j], always).sort && !launch_policy(BIG, CU, others[i], queues[j], never).sort);
    }

  // the number of hardware queues: the library's override, else the runtime's variable, else 4; clamped to 1..32
  CHECK(hardware_queues(nullptr, nullptr) == 4);
  CHECK(hardware_queues(nullptr, "16") == 16 && hardware_queues("", "16") == 16);
  CHECK(hardware_queues("2", "16") == 2 && hardware_queues("2", nullptr) == 2);
  CHECK(hardware_queues("two", "16") == 16 && hardware_queues("2x", "16") == 16 && hardware_queues(" ", "8") == 8);
  CHECK(hardware_queues("two", "many") == 4 && hardware_queues(nullptr, "") == 4 && hardware_queues(nullptr, "4.5") == 4);
  CHECK(hardware_queues("0", "16") == 1 && hardware_queues("-3", nullptr) == 1 && hardware_queues(nullptr, "0") == 1);
  CHECK(hardware_queues("33", nullptr) == 32 && hardware_queues(nullptr, "64") == 32 && hardware_queues("99999999999999999999", "2") == 32);
  CHECK(hardware_queues("32", nullptr) == 32 && hardware_queues("1", nullptr) == 1 && hardware_queues(" 8 ", nullptr) == 8);
  unsetenv("FASTERHIP_HW_QUEUES");
  unsetenv("GPU_MAX_HW_QUEUES");
  CHECK(hardware_queues_from_environment() == 4);
  setenv("GPU_MAX_HW_QUEUES", "16", 1);
  CHECK(hardware_queues_from_environment() == 16);
  setenv("FASTERHIP_HW_QUEUES", "2", 1);
  CHECK(hardware_queues_from_environment() == 2);
  CHECK(std::strcmp(std::getenv("GPU_MAX_HW_QUEUES"), "16") == 0);  // (read, never written)
  setenv("FASTERHIP_HW_QUEUES", "junk", 1);
  CHECK(hardware_queues_from_environment() == 16);
  setenv("GPU_MAX_HW_QUEUES", "junk", 1);
  CHECK(hardware_queues_from_environment() == 4);

  if (failed) {
    std::printf("%d of %d checks failed\n", failed, checks);
    return 1;
  }
  std::printf("ok %d\n", checks);
  return 0;
}
