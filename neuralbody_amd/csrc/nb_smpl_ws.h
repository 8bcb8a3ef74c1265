// nb_smpl_ws.h — the layout of nb_smpl_pose's per-frame workspace `ws` [F, NB_SMPL_WS_FLOATS], for the kernel that writes it
// (nb_smpl.hip) and the one that reads it back (nb_mesh_rig.hip).  Floats of one frame:
//   A [24][12] (rows of the 3x4 relative transforms, less the identity) | pose feature [207] + 1 pad | rot(Rh) [9] | pad
#pragma once
#include "nb_hip.h"

constexpr int WS_A = 0, WS_PF = NB_SMPL_JOINTS * 12, WS_ROT = WS_PF + NB_SMPL_POSE_BASIS + 1, WS_FLOATS = NB_SMPL_WS_FLOATS;
static_assert(WS_ROT + 9 <= WS_FLOATS, "workspace layout");
