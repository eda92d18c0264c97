// mfx_build.h — the traversal BVH built on the GPU (mfx_build.hip).
#ifndef MFX_BUILD_H
#define MFX_BUILD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "mfx_camera_cuts.h"
#include "mfx_layout.h"

// The whole traversal image of a flat scene, built on the current HIP device: a binned-SAH BVH2
// over the primitives (the tree mfx_scene_bvh.cpp's host SahBuilder produces, with its parameters:
// leaves of at most max_leaf primitives, intersection cost c_isect), its BVH4 collapse and the
// layout (nodes renumbered, traversal leaves' slots in depth-first order) — the bytes the host
// path (mfx_scene.cpp: Collapse4 + layout) produces. prim_box: [n][6] conservative FP32 boxes (lo
// xyz, hi xyz); cent: [n][3] centroids; weight: [n] slots per primitive (the intersection cost
// weight); levels: the BVH2's breadth-first levels (kernel launches). Per primitive p the caller gives its slots
// pslots[slot_of[p] .. slot_of[p + 1]) with the reference-leaf box, `first` and the info bits
// other than the shade index already set, their shade records and the reference leaf's ref_blob
// offset.
struct MfxGpuLayoutIn {
    const MfxSlot* pslots;
    const MfxShade* pshade;
    const int32_t* slot_of;   // [n + 1]
    const int32_t* ref16_of;  // [n]
    int32_t nslots;
    int32_t top_nodes;        // nodes numbered breadth-first first (MFX_TOP_NODES), the rest in preorder
};
struct MfxGpuImages {
    std::vector<MfxNode> nodes;
    std::vector<MfxSlot> slots;       // + MFX_LEAF_SLOTS_MAX zero records
    std::vector<int32_t> slot_ref;
    std::vector<MfxShade> shade;
    std::vector<int32_t> shade_of;    // [n] shade index (= slot) of each primitive's first slot
    int32_t max_depth = 0, max_stack = 0, nodes2 = 0, nleaves = 0, levels = 0;
};
hipError_t mfx_gpu_build_images(const float* prim_box, const float* cent, const int32_t* weight, int n, int max_leaf,
                                float c_isect, const MfxGpuLayoutIn& in, MfxGpuImages& out);

// The camera cuts of a flat scene's node image for the camera in device memory (mfx_camera_cuts.h), enqueued on
// st: table[tiles_y * tiles_x][cap] by the routine the host twin (mfx_cut::table_host) runs, so the same
// bytes; stats_dev is zeroed and summed over the tiles. slots: the image's slots, for the per-tile slot cull.
hipError_t mfx_build_cut_table(const MfxNode* nodes, const MfxSlot* slots, const MfxCamera* cam_dev, int W, int H, int cap,
                               MfxCutEntry* table, MfxCutStats* stats_dev, hipStream_t st);

#endif
