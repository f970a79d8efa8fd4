// csrc/rt_room.h's box_face_rule against the resolve trace_flat (rt_device.h) ends with, written out here
// (tests/test_box_face_rule.py): for seeded rays against a box, the rule's distance bits, axis and side must be the
// resolve's on every ray -- called as the resolve calls it, and as the box loop and the resolve share it (the loop
// keeps the axis of an entering ray in two bits, 3 for a ray that starts inside; the resolve recomputes for 3).
// Classes of ray: 0 entering from outside, 1 starting inside, 2 starting exactly on a face plane, 3 aimed exactly at
// an edge (two distances equal bit for bit), 4 aimed exactly at a corner (three equal, or two equal and the third
// within rounding of them), 5 a direction component of exactly zero.
//   box_face_rule [rays per class]  -> one line per class "class c: rays hits ties" and a final "ok <rays> <hits>",
//   or the first mismatches
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_room.h"

namespace {

uint64_t g_state = 0x243F6A8885A308D3ull;
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

// trace_flat's resolve as it stood before the rule (flat_slab's tn, tf, th and the two if-chains)
struct Resolve {
  double th;
  int k, side;
  bool cand;  // the box loop's test before t <= tmax: tf >= max(tn, tmin)
  bool tie;   // two or three per-axis distances equal to the hit's
};
Resolve resolve(const double t0[3], const double t1[3], const double d[3], double tmin) {
  const double tn = std::fmax(std::fmax(std::fmin(t0[0], t1[0]), std::fmin(t0[1], t1[1])), std::fmin(t0[2], t1[2]));
  const double tf = std::fmin(std::fmin(std::fmax(t0[0], t1[0]), std::fmax(t0[1], t1[1])), std::fmax(t0[2], t1[2]));
  Resolve r;
  r.th = tn >= tmin ? tn : tf;
  r.cand = tf >= std::fmax(tn, tmin);
  const bool enter = tn >= tmin;
  int k = 2, same = 0;
  if (enter) {
    if (tn == std::fmin(t0[0], t1[0])) k = 0;
    else if (tn == std::fmin(t0[1], t1[1])) k = 1;
    for (int a = 0; a < 3; a++) same += tn == std::fmin(t0[a], t1[a]);
  } else {
    if (tf == std::fmax(t0[0], t1[0])) k = 0;
    else if (tf == std::fmax(t0[1], t1[1])) k = 1;
    for (int a = 0; a < 3; a++) same += tf == std::fmax(t0[a], t1[a]);
  }
  const double dk = d[k];
  r.k = k;
  r.side = enter ? (dk < 0.0 ? 1 : 0) : (dk < 0.0 ? 0 : 1);
  r.tie = same >= 2;
  return r;
}

}  // namespace

int main(int argc, char** argv) {
  const long per_class = argc > 1 ? std::atol(argv[1]) : 175000;
  const double tmin = 0.001;
  const double lo[3] = {265.0, 0.0, 295.0}, hi[3] = {430.0, 330.0, 460.0};
  long rays = 0, hits = 0, bad = 0;
  for (int cls = 0; cls < 6; cls++) {
    long cls_hits = 0, cls_ties = 0;
    for (long n = 0; n < per_class; n++) {
      double o[3], d[3];
      for (int k = 0; k < 3; k++) d[k] = uni(-1, 1);
      const int ax = (int)(next() % 3), side = (int)(next() & 1);
      switch (cls) {
        case 0:  // from outside, aimed at a point inside
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k] - 600, hi[k] + 600);
          o[ax] = side ? hi[ax] + uni(0.01, 600) : lo[ax] - uni(0.01, 600);
        {
          const double len = uni(0.001, 2);
          for (int k = 0; k < 3; k++) d[k] = (uni(lo[k], hi[k]) - o[k]) * len;
          break;
        }
        case 1:  // from inside
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k], hi[k]);
          break;
        case 2:  // origin exactly on a face plane, inside the face's extent or beside it; going in, out or along
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k] - 30, hi[k] + 30);
          o[ax] = side ? hi[ax] : lo[ax];
          break;
        case 3:    // through an edge: the two axes other than `ax` reach their planes at the same distance bit for bit
        case 4: {  // through a corner: all three, or (every other ray) the third only within rounding
          // |d_k| = a and o_k = e_k - s_k m with m a multiple of 1/8: e_k - o_k = s_k m exactly, and the distance is
          // m * (1 / a) on each such axis, the same product; e_k on either plane and s_k of either sign, so the rays
          // enter by the edge, leave by it from inside, graze it or miss
          const double a = uni(0.05, 1), m = (double)(1 + next() % 4000) / 8.0;
          const bool three = cls == 4 && (n & 1) == 0;
          double e[3];
          for (int k = 0; k < 3; k++) {
            const double s = (next() & 1) ? 1.0 : -1.0;
            e[k] = (next() & 1) ? hi[k] : lo[k];
            d[k] = s * a;
            o[k] = e[k] - s * m;
          }
          if (!three) {
            // cls 3: the third axis crosses anywhere along the edge; cls 4: at the corner, by its own arithmetic
            d[ax] = uni(-1, 1);
            const double p = cls == 3 ? uni(lo[ax], hi[ax]) : e[ax];
            o[ax] = p - d[ax] * (m * (1.0 / a));
          }
          break;
        }
        default:  // a direction component of exactly zero (either sign), the origin sometimes on that axis's plane
          for (int k = 0; k < 3; k++) o[k] = uni(lo[k] - 200, hi[k] + 200);
          d[ax] = side ? 0.0 : -0.0;
          if ((next() & 3) == 0) o[ax] = (next() & 1) ? hi[ax] : lo[ax];
          if ((next() & 3) == 0) d[(ax + 1) % 3] = (next() & 1) ? 0.0 : -0.0;
          if (next() & 1)
            for (int k = 0; k < 3; k++)
              if (k != ax) o[k] = uni(lo[k], hi[k]);
          break;
      }
      double t0[3], t1[3];
      for (int k = 0; k < 3; k++) {
        const double inv = 1.0 / d[k];  // frcp (rt_device.h): IEEE reciprocal, +-inf for +-0
        t0[k] = (lo[k] - o[k]) * inv;
        t1[k] = (hi[k] - o[k]) * inv;
      }
      const Resolve want = resolve(t0, t1, d, tmin);
      // as the resolve calls it
      const rtd::BoxFaceHit<double> f = rtd::box_face_rule<double>(t0, t1, tmin);
      const int f_side = f.enter ? (d[f.axis] < 0.0 ? 1 : 0) : (d[f.axis] < 0.0 ? 0 : 1);
      // as the loop and the resolve share it: two bits from the loop, the rule again for code 3
      const int code = f.enter ? f.axis : 3;
      const bool l_enter = code != 3;
      const int l_axis = l_enter ? code : rtd::box_face_rule<double>(t0, t1, tmin).axis;
      const int l_side = l_enter ? (d[l_axis] < 0.0 ? 1 : 0) : (d[l_axis] < 0.0 ? 0 : 1);
      rays++;
      if (bits(f.t) != bits(want.th) || f.axis != want.k || f_side != want.side || l_axis != want.k ||
          l_side != want.side) {
        if (bad++ < 10)
          std::printf("mismatch class %d: o %.17g %.17g %.17g d %.17g %.17g %.17g: resolve t %.17g axis %d side %d, "
                      "rule t %.17g axis %d side %d, loop form axis %d side %d\n",
                      cls, o[0], o[1], o[2], d[0], d[1], d[2], want.th, want.k, want.side, f.t, f.axis, f_side, l_axis,
                      l_side);
      }
      if (want.cand) cls_hits++, cls_ties += want.tie;
    }
    hits += cls_hits;
    std::printf("class %d: %ld %ld %ld\n", cls, per_class, cls_hits, cls_ties);
  }
  // the float instantiation compiles and agrees on a ray whose distances are exact
  {
    const float t0[3] = {1.0f, 2.0f, -0.5f}, t1[3] = {3.0f, 4.0f, 1.5f};  // tn = 2 (y), tf = 1.5: a miss, still y
    const rtd::BoxFaceHit<float> f = rtd::box_face_rule<float>(t0, t1, 0.001f);
    const float u0[3] = {-1.0f, -2.0f, -0.5f};  // inside: tf = 1.5 (z)
    const rtd::BoxFaceHit<float> g = rtd::box_face_rule<float>(u0, t1, 0.001f);
    if (!f.enter || f.axis != 1 || f.t != 2.0f || g.enter || g.axis != 2 || g.t != 1.5f) {
      std::printf("float: enter %d axis %d t %g; enter %d axis %d t %g\n", (int)f.enter, f.axis, (double)f.t,
                  (int)g.enter, g.axis, (double)g.t);
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
