// The slice plan of the MANO kernel (csrc/mano.hip), stated once for launch_mano and for the kernel: how many workgroups
// share a hand and which vertices each of them owns.  Plain C++, no HIP (constexpr functions are callable from device
// code as they stand): tools/mano_plan_check.cpp compiles it alone and tests/test_mano_plan_host.py holds it to its rules.
//
// A hand is split over `slices` workgroups by vertex range.  Everything before the pose blend is repeated per slice;
// pose blend, skinning and the outputs of vertex v belong to the one slice whose range holds v, a fingertip joint to the
// slice that skinned its vertex, the 16 chain joints and the center to slice 0.
#pragma once

namespace acrmi {

constexpr int NV = 778, NV3 = 2334;

// The five fingertip vertices (mano/manolayer.py:244-247), thumb to little finger, [left, right]: the initialiser of the
// device table (csrc/mano_stages.h's mano_tips, beside the rest of the kinematic tree) and of the host's.
#define ACRMI_MANO_TIPS {{745, 317, 445, 556, 673}, {745, 317, 444, 556, 673}}
constexpr int MANO_TIPS[2][5] = ACRMI_MANO_TIPS;

constexpr int MANO_MAX_SLICES = 8;
constexpr int MANO_SLICED_BELOW = 256;   // hands per call from which on a hand is one workgroup

// Workgroups per hand of a call of H >= 1 hands: enough to give every CU one (2 hands: 8 slices; 128 hands: 2).  A root
// joint that is a FINGERTIP (center_idx 4, 8, 12, 16, 20: a skinned vertex, mano/manolayer.py:241-262) is known only to the
// slice that skinned it: one slice then.
constexpr int mano_slices(int H, int center_idx) {
  const bool tip_center = center_idx >= 0 && center_idx % 4 == 0 && center_idx > 0;
  return tip_center ? 1
                    : (H >= MANO_SLICED_BELOW ? 1 : (MANO_SLICED_BELOW / H > MANO_MAX_SLICES ? MANO_MAX_SLICES : MANO_SLICED_BELOW / H));
}

// Vertices [*v0, *v1) of slice `slice` of `slices`: ceil(NV / slices) each, the last one what is left.
constexpr void mano_slice_range(int slice, int slices, int* v0, int* v1) {
  const int vper = (NV + slices - 1) / slices;
  *v0 = slice * vper;
  *v1 = *v0 + vper < NV ? *v0 + vper : NV;
}

}  // namespace acrmi
