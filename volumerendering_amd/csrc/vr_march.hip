// vr_march.hip -- the march kernels with the per-sample multiply-adds rounded separately (VR_FUSED = 0, namespace vr): the default
// normative arithmetic, a * b + c as a rounded product and a rounded sum.  vr_fused.hip is the same text in the other mode.
// A translation unit of its own, apart from the C ABI (vr_api.hip), which reaches it through the four entry points that
// vr_device.h declares: an edit to the ABI, an auxiliary kernel or a voxel tool recompiles no march kernel.
#define VR_KNS vr
#define VR_FUSED 0
#include "vr_launch.h"
