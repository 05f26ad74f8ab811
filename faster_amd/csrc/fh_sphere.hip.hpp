// fh_sphere.hip.hpp — getIntersectionWithSphere (faster/src/utils.cpp:713-776) on the device, once: the path search clips its paths
// with it (fh_path.hip.hpp, in fh_map.hip) and the safe corridor marches through known space with it (fh_safe.hip.hpp, in
// fh_capi.hip).  Includes nothing of the project.
//
// The host has its own copy, fhfront::sphere_crossing (host/corridor_frontend.hpp), with the same expressions — on purpose: it is
// what the device is tested against bit for bit (the front-end parity tests), and one function shared by host and device would make
// that comparison a tautology.
#pragma once
#include <hip/hip_runtime.h>

namespace fhs {

// one root of |A + t (B - A) - c| = r, the point at it in `out`; returns the discriminant.  The reference's arithmetic: single
// precision, except that pow(float, 2) is a double (the squares are summed in double, rounded once) and `- r * r` is a double
// subtraction.  No fused multiply-adds: every product and sum rounds as on the host.
__device__ inline float sphere_root(const double A[3], const double B[3], double r, const double c[3], double out[3]) {
#pragma clang fp contract(off)
  const float x1 = (float)A[0], y1 = (float)A[1], z1 = (float)A[2], x2 = (float)B[0], y2 = (float)B[1], z2 = (float)B[2];
  const float x3 = (float)c[0], y3 = (float)c[1], z3 = (float)c[2];
  const float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
  const float a = (float)((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
  const float b = 2.0f * (dx * (x1 - x3) + dy * (y1 - y3) + dz * (z1 - z3));
  const float cf = x3 * x3 + y3 * y3 + z3 * z3 + x1 * x1 + y1 * y1 + z1 * z1 - 2.0f * (x3 * x1 + y3 * y1 + z3 * z1);
  const float cc = (float)((double)cf - r * r);
  const float disc = b * b - 4.0f * a * cc;
  const float t = (-b + sqrtf(disc)) / (2.0f * a);
  out[0] = (double)(x1 + dx * t); out[1] = (double)(y1 + dy * t); out[2] = (double)(z1 + dz * t);
  return disc;
}
// point where the segment a -> b leaves the sphere (centre c, radius r)
__device__ inline void sphere_crossing(const double a[3], const double b[3], double r, const double c[3], double out[3]) {
  if (sphere_root(a, b, r, c, out) <= 0) sphere_root(c, a, r, c, out);  // tangent / no crossing: the ray centre -> a
}

}  // namespace fhs
