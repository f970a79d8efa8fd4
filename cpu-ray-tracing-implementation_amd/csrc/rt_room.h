// rt_room.h -- the closest hit of a ray on the faces of an axis-aligned box of which some exist (a room: the five
// walls of a Cornell box are the faces of [0, 555]^3 with one missing), decided from the six slab distances alone.
// A pure function with no HIP in it: trace_flat (rt_device.h) calls it on the device, and a plain C++ program
// compares it with one quad test per face (tests/native/room_rule.cpp).
//
// Face 2k + s lies on plane lo_k (s = 0) or hi_k (s = 1) of axis k, as FlatBoxT::face. The caller computes
//   t0[k] = (lo_k - o_k) * inv_k,  t1[k] = (hi_k - o_k) * inv_k
// which are the very expressions of the quad test's distance (flat_quad_test's th), so a hit's t has the quad
// test's bits. With tn the largest per-axis near distance and tf the smallest per-axis far distance:
//   - a candidate exists only if tf >= max(tn, tmin);
//   - tn >= tmin and the face the ray enters through exists: the hit is tn on that face;
//   - else the face the ray leaves through exists: the hit is tf on that face;
//   - else nothing.
// The caller then applies t <= tmax. With all six faces this is flat_slab's rule (rt_device.h).
//
// Which face that is: tn and tf are each one of the six distances, so the face is the plane whose distance is
// the hit's t bit for bit -- the first axis (x, y, z) that has such a plane, hi_k if it is t1[k]. Two planes
// share a distance only where the ray passes through an edge of the box within rounding, where the quad tests
// decide by rounding too.
// At most one face may be absent (present has five or six bits): an absent face is entered (left) through when
// tn (tf) equals that face's own distance.
// NaN distances (origin on a plane, direction component zero) drop out of fmin / fmax as in flat_slab.
#pragma once

#include <math.h>
#include <stdint.h>

#if !defined(__HIP__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace rtd {

constexpr uint32_t kRoomAllFaces = 63u;

// the one absent face of a present mask (6: none); masks with fewer than five faces are not rooms
__host__ __device__ inline uint32_t room_absent(uint32_t present) {
  uint32_t f = 0;
  while (f < 6u && ((present >> f) & 1u)) f++;
  return f;
}
__host__ __device__ inline bool room_mask_ok(uint32_t present) {
  const uint32_t miss = ~present & kRoomAllFaces;
  return (present & ~kRoomAllFaces) == 0 && (miss & (miss - 1u)) == 0;
}

template <class R>
struct RoomHit {
  bool hit;  // before the caller's t <= tmax
  R t;       // meaningful when hit
  int face;  // 2k + s, meaningful when hit
};

template <class R>
__host__ __device__ inline RoomHit<R> room_rule(const R t0[3], const R t1[3], uint32_t present, R tmin) {
  const R n0 = fmin(t0[0], t1[0]), n1 = fmin(t0[1], t1[1]), n2 = fmin(t0[2], t1[2]);
  const R f0 = fmax(t0[0], t1[0]), f1 = fmax(t0[1], t1[1]), f2 = fmax(t0[2], t1[2]);
  const R tn = fmax(fmax(n0, n1), n2);
  const R tf = fmin(fmin(f0, f1), f2);
  // the absent face's own distance against tn and tf; the switch is on a value every ray of a launch shares
  bool in_absent = false, out_absent = false;
  switch (room_absent(present)) {
    case 0: in_absent = tn == t0[0], out_absent = tf == t0[0]; break;
    case 1: in_absent = tn == t1[0], out_absent = tf == t1[0]; break;
    case 2: in_absent = tn == t0[1], out_absent = tf == t0[1]; break;
    case 3: in_absent = tn == t1[1], out_absent = tf == t1[1]; break;
    case 4: in_absent = tn == t0[2], out_absent = tf == t0[2]; break;
    case 5: in_absent = tn == t1[2], out_absent = tf == t1[2]; break;
    default: break;
  }
  const bool enter = (tn >= tmin) & !in_absent;
  RoomHit<R> r;
  r.hit = (tf >= fmax(tn, tmin)) & (enter | !out_absent);
  r.t = enter ? tn : tf;
  // the face: the first axis with a plane at exactly the hit distance, and which of its two planes that is
  // (compares and mask logic only: no lane takes a branch)
  const bool l0 = t0[0] == r.t, h0 = t1[0] == r.t, l1 = t0[1] == r.t, h1 = t1[1] == r.t, h2 = t1[2] == r.t;
  const bool a0 = l0 | h0, a1 = l1 | h1;
  const bool hi = (a0 & h0) | (!a0 & a1 & h1) | (!a0 & !a1 & h2);
  r.face = (a0 ? 0 : (a1 ? 2 : 4)) + (hi ? 1 : 0);
  return r;
}

// The face of a closed box (flat_slab's rule, rt_device.h) from the same six distances: the hit is tn through the
// face the ray enters by when tn >= tmin, else tf through the face it leaves by (a ray that starts inside). The
// axis is the first of x, y, z whose near (far) distance is tn (tf) bit for bit, z when neither x nor y is: at an
// edge or a corner, where two or three are equal, the first wins, and a NaN distance equals nothing. Which of the
// axis's two planes it is the caller reads from the sign of the direction. trace_flat's box loop and its resolve
// both call this (the loop keeps the axis of an entering hit, so the resolve computes nothing for it), and
// tests/native/box_face_rule.cpp compares it with the resolve written out.
template <class R>
struct BoxFaceHit {
  R t;         // tn or tf (the caller tests tf >= max(tn, tmin) and t <= tmax)
  int axis;    // 0, 1, 2
  bool enter;  // tn >= tmin
};
template <class R>
__host__ __device__ inline BoxFaceHit<R> box_face_rule(const R t0[3], const R t1[3], R tmin) {
  const R n0 = fmin(t0[0], t1[0]), n1 = fmin(t0[1], t1[1]), n2 = fmin(t0[2], t1[2]);
  const R f0 = fmax(t0[0], t1[0]), f1 = fmax(t0[1], t1[1]), f2 = fmax(t0[2], t1[2]);
  const R tn = fmax(fmax(n0, n1), n2);
  const R tf = fmin(fmin(f0, f1), f2);
  BoxFaceHit<R> r;
  r.enter = tn >= tmin;
  r.t = r.enter ? tn : tf;
  const int an = tn == n0 ? 0 : (tn == n1 ? 1 : 2), af = tf == f0 ? 0 : (tf == f1 ? 1 : 2);
  r.axis = r.enter ? an : af;
  return r;
}

}  // namespace rtd
