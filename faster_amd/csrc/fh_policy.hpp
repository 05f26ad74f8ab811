// fh_policy.hpp — how a solve launch is scheduled, decided on the host from what is known when it is issued.  Host only, no HIP
// includes: fh_capi.hip (launch_solve) is its one caller in the library, tests/cpp/test_launch_policy.cpp checks the table with g++.
//
// What decides is how many solve launches of the process can really run side by side on the device.  That is the number of hardware
// queues the HIP runtime opens (GPU_MAX_HW_QUEUES; 4 unless the variable says otherwise), not the number of streams: streams beyond it
// share a queue, and launches of one queue run one after the other.  Three regimes:
//   alone          no other context of the process has a solve launch in flight on the device.  What ends the launch is its tail (a few
//                  long trees on one wavefront each): look around often, start the hardest corridors first.
//   beside others  others are in flight, and there is a hardware queue for every one of them and for this launch.  The tail is hidden
//                  behind the bulk of the others: look around half as often, no launch order.
//   queued         more launches are outstanding than there are hardware queues: this launch will wait behind another one, and others
//                  will wait behind it.  Its tail holds a queue that the launches behind it could use — but with four launches really
//                  running the tail is hidden as well as with fourteen, and the choices are those of `beside others`.
// Blind spots: launches of OTHER processes on the device are not seen, and a runtime whose queue count differs from what the variable
// says (a build with another default, a variable set after the runtime read it) is believed to have what the variable says;
// FASTERHIP_HW_QUEUES states the real number for such a caller.  The library only reads these variables.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cstdlib>

#include "../../include/fasterhip.h"

// The look periods of the first two regimes (fh_sched.look_every = 0); fh_solve.hip.hpp names the same two values for its comments.
#ifndef FH_LOOK_EVERY
#define FH_LOOK_EVERY 8
#endif
#ifndef FH_LOOK_EVERY_BUSY
#define FH_LOOK_EVERY_BUSY 16
#endif
// The queued regime's choices.  Measured on C4 with 14 pipelines on 4 hardware queues, four launches really running at once
// (profiles/r10_knob_survey.txt): nothing beats what a launch beside others does — a period of 8 is -4.6 %, 32 is +0.9 % with
// overlapping ranges, the launch order -0.9 %, 8 / 16 waiting workgroups -0.2 / -1.8 % — so the values are those of that regime; they
// have names of their own because the regime is where a caller's streams outnumber the queues, and is measured separately.
namespace fhp {

constexpr int LOOK_EVERY_QUEUED = FH_LOOK_EVERY_BUSY;
constexpr bool ORDER_WHEN_QUEUED = false;     // true: a queued launch of >= ORDER_MIN_UNITS units is sorted (fh_sched.launch_order = 1)
constexpr int WAITING_CU_DIVISOR_QUEUED = 64;  // waiting workgroups of a big queued batch: CUs / this
constexpr int ORDER_MIN_UNITS = 2048;          // smaller batches are never sorted: the two sorting launches cost more than the order gains

enum Regime { ALONE = 0, BESIDE_OTHERS = 1, QUEUED = 2 };

constexpr int QUEUES_DEFAULT = 4, QUEUES_MAX = 32;  // HIP's own default; the most this library believes

// `others`: solve launches of other contexts of the process in flight on the device; `queues`: hardware queues of the runtime
inline Regime regime_of(int others, int queues) { return others <= 0 ? ALONE : (others + 1 <= queues ? BESIDE_OTHERS : QUEUED); }

// A queue count as a variable states it: a decimal integer with nothing behind it, clamped to 1..QUEUES_MAX.  False: not a number.
inline bool parse_queues(const char* text, int* out) {
  if (!text || !*text) return false;
  char* end = nullptr;
  errno = 0;
  const long v = std::strtol(text, &end, 10);
  if (end == text) return false;
  while (*end == ' ' || *end == '\t') end++;
  if (*end) return false;
  *out = errno == ERANGE ? (v < 0 ? 1 : QUEUES_MAX) : (int)std::min<long>(std::max<long>(v, 1), QUEUES_MAX);
  return true;
}
// The library's override first, else the variable the runtime reads, else the runtime's default (an unparsable value counts as absent)
inline int hardware_queues(const char* override_text, const char* runtime_text) {
  int q = QUEUES_DEFAULT;
  if (parse_queues(override_text, &q) || parse_queues(runtime_text, &q)) return q;
  return QUEUES_DEFAULT;
}
inline int hardware_queues_from_environment() { return hardware_queues(std::getenv("FASTERHIP_HW_QUEUES"), std::getenv("GPU_MAX_HW_QUEUES")); }

struct LaunchPolicy {
  Regime regime;
  int look_every;          // nodes of a tree between two looks at the control words
  bool sort;               // start the hardest corridors first (the two order launches)
  int waiting_workgroups;  // workgroups that keep waiting for frames when the fresh problems run out
  int publish_factor;      // publish-ahead: the multiple of the mean iteration count from which a problem publishes ahead (0: never)
  int backlog;             //                frames that may be published ahead of the takers
};

// One solve launch of n units on a device with n_cu compute units.  A non-zero field of `s` wins over the automatic choice
// (publish_factor and backlog have no automatic value: 0 means off, fh_default_sched sets 4 and 32).
inline LaunchPolicy launch_policy(int n, int n_cu, int others, int queues, const fh_sched& s) {
  LaunchPolicy p;
  p.regime = regime_of(others, queues);
  const bool queued = p.regime == QUEUED;
  p.look_every = s.look_every > 0 ? s.look_every : (p.regime == ALONE ? FH_LOOK_EVERY : (queued ? LOOK_EVERY_QUEUED : FH_LOOK_EVERY_BUSY));
  p.sort = n >= ORDER_MIN_UNITS && (s.launch_order >= 2 || (s.launch_order == 1 && (p.regime == ALONE || (queued && ORDER_WHEN_QUEUED))));
  // (a batch of up to 8 problems per CU — one vehicle's replan: one problem and a helper workgroup per CU — keeps CUs / 16: its helpers ARE the waiters)
  p.waiting_workgroups = s.waiting_workgroups > 0 ? s.waiting_workgroups
                                                  : (n <= 8 * n_cu ? std::max(8, n_cu / 16) : std::max(2, n_cu / (queued ? WAITING_CU_DIVISOR_QUEUED : 64)));
  p.publish_factor = s.publish_factor;
  p.backlog = s.backlog;
  return p;
}

}  // namespace fhp
