// mfx_scene.h — host-side scene preparation (runs once per `Scene`, Scene.fs:298-313).
#ifndef MFX_SCENE_H
#define MFX_SCENE_H

#include <string>
#include <vector>

#include "../../include/mafrix_rt.h"
#include "mfx_layout.h"
#include "mfx_texture.h"

struct MfxHostScene {
    // reference heap-BVH leaf grouping (BvhNode.fs:24-61)
    std::vector<int32_t> ref_indices;                  // `indices` after Subdivide
    std::vector<int32_t> leaf_first, leaf_count;       // leaves in heap (DFS) order
    // device images
    std::vector<MfxNode> nodes;     // BVH4 over primitives (preorder)
    std::vector<MfxSlot> slots;     // traversal leaves: runs of MfxSlot records, DFS order
    std::vector<int32_t> slot_ref;  // per slot: 16-byte offset of its reference leaf in ref_blob
    std::vector<uint8_t> ref_blob;  // reference leaves: MfxLeaf headers + slot copies, heap order
    std::vector<MfxShade> shade;    // per traversal slot, in slots[] order
    std::vector<MfxInstance> inst;  // two-level scenes: instances traced through a template BVH
    int32_t nclusters = 0;          // reference leaves
    int32_t ntleaves = 0;           // traversal leaves
    int32_t world_slots = 0;        // slots of the world primitives (what a flat image holds)
    int32_t tlas_nodes = 0, blas_nodes = 0, blas_slots = 0, ntemplates = 0, top_slots = 0;  // two-level shape (blas_slots: one run per template)
    std::vector<double> albedo;  // [nmat][3]
    MfxLight light;                // lights[0]: what the one-light kernel instances and the megakernel read
    std::vector<MfxLight> lights;  // L_0 .. L_{N-1} (mfx_create_lights; N == 1: {light}), pdf = (1 / area) / N
    MfxCamera camera;
    int32_t width = 0, height = 0, max_depth = 3;
    int32_t bvh_depth = 0;     // longest root-to-leaf path in nodes[]
    int32_t stack_entries = 1; // traversal stack bound: pushes along any root-to-node path
    float eps = 0.f;           // conservative box widening
    float eps_templates = 0.f; // two-level scenes: the widening of the template BVHs' boxes (0: a flat image)
    // what eps is sized by, less the camera (mfx_camera_eps): R over the primitives and the light, the
    // scene box, and the largest |offset| coordinate of the traced instances
    double extent_R0 = 0.0, box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0}, inst_offmax = 0.0;
    // How far beyond tMax a query's node tests must still enter boxes until its first hit.
    // A reference leaf whose box is entered before tMax and whose primitives are all hit beyond tMax is
    // a hit (Triangle.Hit ignores tMax; the leaf's minBy then has no miss key), and the traversal finds
    // it through one of those primitives' own boxes, which may be entered only after tMax: later than
    // the leaf's box by at most its diagonal (unit directions), by nothing when one primitive's box is
    // the leaf's. The largest such distance over the reference leaves, rounded up.
    double tslack = 0.0;
    // build record (mfx_build_info)
    bool bvh_gpu = false;      // traversal BVH2 built on the GPU (mfx_build.hip)
    bool images_gpu = false;   // and its BVH4 collapse and image layout too (flat scenes)
    int32_t bvh_levels = 0;    // its breadth-first levels (GPU) / depth + 1 (host)
    int32_t nodes2 = 0;        // its internal nodes
    double ms_ref_bvh = 0, ms_bvh = 0, ms_total = 0;
};

// Builds everything from the C-ABI scene description; returns false with `err` set on bad input.
// gpu_bvh: build the traversal BVH2 on the current HIP device (the same tree as the host build).
// instances (mfx_create_instanced): d->prims are templates, the world scene is their expansion;
// flatten: trace it through one flat BVH instead of two levels.
// lights (mfx_create_lights): the lights that replace d->light, which is then not read, with what
// mfx_prepare_lights made of them (prepared->size() of them; the caller validates them there, once).
bool mfx_build_scene(const mfx_scene_desc* d, MfxHostScene& s, std::string& err, bool gpu_bvh = false,
                     const mfx_instance* instances = nullptr, int ninstances = 0, bool flatten = false,
                     const mfx_quad_light* lights = nullptr, const std::vector<MfxLight>* prepared = nullptr);
// The lights of a context as the kernels read them (Light.fs:31-40): per light the two sample triangles,
// area and pdf = (1 / area) / N. False with `err` set: a count outside 1 .. MFX_MAX_LIGHTS, a non-finite
// field (err names the light's index), and with N >= 2 an area that is 0 or not finite.
bool mfx_prepare_lights(const mfx_quad_light* lights, int nlights, std::vector<MfxLight>& out, std::string& err);
// Albedo textures of a context (mfx_create_textured; mfx_texture.cpp), as the host prepares them: beside the
// scene images, never part of them (mfx_scene_digest does not cover them, MfxShade and the slots are as ever).
struct MfxTexHost {
    std::vector<MfxTexDesc> desc;  // per texture: its first texel in the concatenation, width, height
    std::vector<double> uvrec;     // [world primitives][8] the UV records (zeros for an untextured primitive)
    std::vector<int32_t> ptex;     // [world primitives] the primitive's texture, -1: untextured
    int64_t ntexels = 0;
    bool on = false;               // some world primitive is textured: the textured kernel instances run
};
// The descriptors of textures[0..ntextures), from the sizes alone. False with `err` naming the first offender:
// a count outside 0 .. MFX_MAX_TEXTURES, a width or height outside 1 .. MFX_MAX_TEXTURE_DIM, too many texels.
bool mfx_texture_descs(const mfx_texture* textures, int ntextures, std::vector<MfxTexDesc>& desc, int64_t& ntexels,
                       std::string& err);
// Everything mfx_create_textured refuses about textures and maps, then the UV table of the world primitives
// (scene->prims, or their expansion by `instances`). out.on == false: an untextured scene.
bool mfx_prepare_textures(const mfx_scene_desc* scene, const mfx_instance* instances, int ninstances,
                          const mfx_texture* textures, int ntextures, const mfx_prim_uv* prim_uv, MfxTexHost& out,
                          std::string& err);
// PinholeCamera's constructor (Camera.fs:122-133), or with c.derived the fields as they are.
void mfx_derive_camera(const mfx_pinhole& c, MfxCamera& cam);
// The widening mfx_build_scene would give s's boxes with the camera at pos: (float)ldexp(R + T, -19), and
// for a two-level image its template BVHs' (0 for a flat one). Boxes built with at least these stay
// conservative for every ray that camera starts.
void mfx_camera_eps(const MfxHostScene& s, const double* pos, float* eps, float* eps_templates);
// The world primitive list of an instanced scene (mfx_instance: template + offset, FP64).
bool mfx_expand(const mfx_prim* prims, int64_t nprims, const mfx_instance* inst, int ninst,
                std::vector<mfx_prim>& world, std::string& err);
// FNV-1a over the device images (nodes, slots, slot_ref, ref_blob, shade, inst) and, with several lights,
// the light table: mfx_build_info's digest.
uint64_t mfx_scene_digest(const MfxHostScene& s);

#endif
