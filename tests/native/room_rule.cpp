// csrc/rt_room.h's rule against brute force (tests/test_room_rule.py): for seeded rays and every present mask
// with five or six faces, the closest hit among one quad test per existing face -- the arithmetic of
// rt_device.h flat_quad_test, in double -- must be the rule's face with the same bits of t.
//   room_rule [rays per mask]   -> one line per mask and a final "ok <rays> <hits>", or the first mismatches
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "rt_room.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
double uni(double a, double b) { return a + (b - a) * uni(); }

uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}

// flat_quad_test (rt_device.h) for the face on plane `plane` of axis A, spanning [lo, hi] in the two others
bool quad_test(int A, double plane, const double lo[3], const double hi[3], const double o[3], const double d[3],
               const double inv[3], double tmin, double tmax, double& th) {
  const int U = A == 0 ? 1 : 0, W = A == 2 ? 1 : 2;
  th = (plane - o[A]) * inv[A];
  const double a = std::fma((o[U] + th * d[U]) - lo[U], 1.0 / (hi[U] - lo[U]), 0.0);
  const double b = std::fma((o[W] + th * d[W]) - lo[W], 1.0 / (hi[W] - lo[W]), 0.0);
  const bool in_t = (th >= tmin) & (th <= tmax);
  const bool in_ab = (bits(a) <= 0x3FF0000000000000ull) & (bits(b) <= 0x3FF0000000000000ull);
  return in_t & in_ab;
}

}  // namespace

int main(int argc, char** argv) {
  const long per_mask = argc > 1 ? std::atol(argv[1]) : 150000;
  const double tmin = 0.001, inf = std::numeric_limits<double>::infinity();
  const double lo[3] = {0.0, -20.0, 100.0}, hi[3] = {555.0, 535.0, 655.5};
  long rays = 0, hits = 0, bad = 0;
  for (int miss = -1; miss < 6; miss++) {  // the closed box, then each open face
    const uint32_t present = miss < 0 ? 63u : 63u & ~(1u << miss);
    if (!rtd::room_mask_ok(present) || rtd::room_absent(present) != (miss < 0 ? 6u : (uint32_t)miss)) {
      std::printf("mask %u: room_absent / room_mask_ok wrong\n", present);
      return 1;
    }
    long mask_hits = 0, by_class[5] = {0, 0, 0, 0, 0};
    for (long n = 0; n < per_mask; n++) {
      const int cls = (int)(n % 5);
      double o[3], d[3];
      for (int k = 0; k < 3; k++) d[k] = uni(-1, 1);
      const int ax = (int)(next() % 3), side = (int)(next() & 1);
      switch (cls) {
        case 0:  // from inside
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k], hi[k]);
          break;
        case 1:  // from outside, aimed at a point inside: enters through the back of a face, or the opening
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k] - 900, hi[k] + 900);
          o[ax] = side ? hi[ax] + uni(0.01, 900) : lo[ax] - uni(0.01, 900);
          for (int k = 0; k < 3; k++) d[k] = uni(lo[k], hi[k]) - o[k];
          break;
        case 2:  // from inside toward the opening (the closed box: toward face `ax, side`)
        {
          const int f = miss < 0 ? 2 * ax + side : miss;
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k], hi[k]);
          double p[3];
          for (int k = 0; k < 3; k++) p[k] = uni(lo[k] - 50, hi[k] + 50);  // some just miss the opening
          p[f >> 1] = (f & 1) ? hi[f >> 1] : lo[f >> 1];
          for (int k = 0; k < 3; k++) d[k] = (p[k] - o[k]) * uni(0.5, 3);
          break;
        }
        case 3:  // origin exactly on a wall plane (inside the wall's extent or beside it)
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k] - 30, hi[k] + 30);
          o[ax] = side ? hi[ax] : lo[ax];
          break;
        default:  // a direction component of exactly zero (either sign of zero), origin anywhere
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k] - 300, hi[k] + 300);
          d[ax] = side ? 0.0 : -0.0;
          if (next() & 1) d[(ax + 1) % 3] = (next() & 1) ? 0.0 : -0.0;
          break;
      }
      double inv[3], t0[3], t1[3];
      for (int k = 0; k < 3; k++) {
        inv[k] = 1.0 / d[k];  // frcp (rt_device.h): IEEE reciprocal, +-inf for +-0
        t0[k] = (lo[k] - o[k]) * inv[k];
        t1[k] = (hi[k] - o[k]) * inv[k];
      }
      // brute force: the faces in any order, ties to the later one (none occur between faces off the edges)
      double tmax = inf;
      int face = -1;
      for (int f = 0; f < 6; f++) {
        if (!((present >> f) & 1u)) continue;
        double th;
        if (quad_test(f >> 1, (f & 1) ? hi[f >> 1] : lo[f >> 1], lo, hi, o, d, inv, tmin, tmax, th)) tmax = th, face = f;
      }
      const rtd::RoomHit<double> r = rtd::room_rule<double>(t0, t1, present, tmin);
      const bool hit = r.hit && r.t <= inf;
      rays++;
      if (hit != (face >= 0) || (hit && (r.face != face || bits(r.t) != bits(tmax)))) {
        if (bad++ < 10)
          std::printf("mismatch mask %u class %d: o %.17g %.17g %.17g d %.17g %.17g %.17g: quads face %d t %.17g, "
                      "rule hit %d face %d t %.17g\n",
                      present, cls, o[0], o[1], o[2], d[0], d[1], d[2], face, tmax, (int)r.hit, r.face, r.t);
      }
      if (face >= 0) mask_hits++, by_class[cls]++;
    }
    hits += mask_hits;
    std::printf("mask %2u: %ld rays, hits by class %ld %ld %ld %ld %ld\n", present, per_mask, by_class[0], by_class[1],
                by_class[2], by_class[3], by_class[4]);
  }
  // the float instantiation compiles and agrees with double on a ray whose distances are exact in both
  {
    const float t0[3] = {-1.0f, -2.0f, -0.5f}, t1[3] = {3.0f, 2.0f, 1.5f};
    const rtd::RoomHit<float> r = rtd::room_rule<float>(t0, t1, 63u & ~(1u << 5), 0.001f);
    const rtd::RoomHit<float> q = rtd::room_rule<float>(t0, t1, 63u, 0.001f);
    if (r.hit || !q.hit || q.face != 5 || q.t != 1.5f) {
      std::printf("float: open %d, closed %d face %d t %g\n", (int)r.hit, (int)q.hit, q.face, (double)q.t);
      return 1;
    }
  }
  if (bad) {
    std::printf("FAILED: %ld of %ld rays\n", bad, rays);
    return 1;
  }
  std::printf("ok %ld %ld\n", rays, hits);
  return 0;
}
