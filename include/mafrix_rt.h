/*
 * mafrix_rt.h — C ABI of the MI355X (gfx950) path-tracing hot path.
 *
 * This is the drop-in boundary for NAIVEddd/MafrixRaytracing's F# EngineCore hot path:
 * the F# `Scene` constructor and `Scene.Render` (EngineCore/Scene/Scene.fs:298-333) bind these
 * entry points through P/Invoke instead of running `PixelIntegrator`
 * (EngineCore/Core/Integrator/Integrators.fs:143-172) on the .NET thread pool.
 *
 * Conventions
 *  - extern "C", cdecl, plain pointers and sizes, no C++ or torch types.
 *  - Every struct is blittable (sequential layout, natural alignment) so .NET can pin it.
 *  - Return value: 0 on success, a negative MFX_E_* code on failure; mfx_last_error()
 *    gives a thread-local message. Nothing ever falls back to a CPU path.
 *  - One mfx_ctx is driven by one host thread at a time (the reference calls Sample from its
 *    single render thread, Film.fs:32, and fans out internally, Integrators.fs:164).
 *  - All calls are synchronous: when a call returns, its output buffer is complete.
 *
 * Numerics contract: every decision the reference makes in FP64
 * (camera ray, AABB slab test, Möller–Trumbore, sphere roots, rejection-sampled hemisphere,
 * light sample point, shadow distance) is made in FP64 with the reference's operation order
 * and no FMA contraction, so GPU paths follow the CPU oracle's paths bit for bit; the
 * BVH traversal that *finds* candidate leaves runs in FP32 with conservatively widened boxes.
 */
#ifndef MAFRIX_RT_H
#define MAFRIX_RT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFX_ABI_VERSION 6  /* 6: device lists partition the film by tile rows; MFX_F_ROW_PARTITION */
#define MFX_MAX_DEVICES 64
#define MFX_MAX_RENDER_AHEAD 1024
#define MFX_MAX_LIGHTS 64 /* lights of a context at most (mfx_create_lights; ABI 6, additive) */

/* error codes */
#define MFX_OK 0
#define MFX_E_INVALID (-1)   /* bad argument / malformed scene */
#define MFX_E_DEVICE (-2)    /* HIP runtime error, no device, kernel fault */
#define MFX_E_NOMEM (-3)     /* host or device allocation failed */
#define MFX_E_STATE (-4)     /* call out of order (e.g. render before create) */

/* Primitive kinds: the three IHitable structs the reference's Bvh holds (BvhNode.fs:24). */
#define MFX_PRIM_TRIANGLE 0  /* Triangle(v0,v1,v2,mat)        Core/Shape/Trangle.fs:107-119 */
#define MFX_PRIM_RECT 1      /* Rect(v0,v1,v2,v3,mat) = two triangles (v0,v1,v2),(v0,v2,v3)  Rect.fs:11-20 */
#define MFX_PRIM_SPHERE 2    /* Sphere(center,radius,mat)     Core/Shape/Sphere.fs:9-16 */

/* One primitive of the scene, in the order of Scene state.shapes (Scene.fs:168-177, 301).
 * The order matters: it is the index space Bvh.Build sorts (BvhNode.fs:25).
 *  TRIANGLE: p[0..2] = v0,v1,v2
 *  RECT:     p[0..3] = v0,v1,v2,v3 (the four OBJ face vertices, ObjModelLoader.fs:84-89)
 *  SPHERE:   p[0] = center, p[1][0] = radius                                              */
typedef struct mfx_prim {
    int32_t kind;
    int32_t material; /* index into mfx_scene_desc.albedo (MaterialManager order, IMaterial.fs:20-35) */
    double p[4][3];
} mfx_prim; /* 104 bytes */

/* NewAreaLight(p0,p1,p2,p3,normal,intensity) (Core/Lights/Light.fs:31-40), as built by
 * Scene.fs:193 from a Rect: (trig1.v0, trig1.v1, trig1.v2, trig2.v2, trig1.normal, I). */
typedef struct mfx_quad_light {
    double p[4][3];
    double normal[3];
    double intensity[3];
} mfx_quad_light;

/* PinholeCamera(pos, dir, fov, aspectRatio) (Core/Camera.fs:122-133). With derived == 0 the
 * library runs the constructor (CameraCoordinate + tan); with derived != 0 it takes an existing
 * camera's fields as they are — PinholeCamera.position, .topleft, .coord.right, .coord.down —
 * which is what the F# shim passes, so GetRay (Camera.fs:134-139) starts from identical bits. */
typedef struct mfx_pinhole {
    double position[3];
    double direction[3];
    double fov;    /* degrees, as in Scene.xml; effective horizontal FOV is fov/2 (Camera.fs:125) */
    double aspect; /* aspectratio attribute; NOT derived from the film size (Scene.fs:61-72) */
    double topleft[3], right[3], down[3];
    int32_t derived;
    int32_t reserved;
} mfx_pinhole;

/* The scene a `Scene` is constructed from (Scene.fs:298-313). Deep-copied by mfx_create. */
typedef struct mfx_scene_desc {
    const mfx_prim* prims;
    int64_t nprims;
    const double* albedo; /* [nmat][3] Lambert albedo per MaterialManager slot (Material.fs:29-37);
                             Metal -> its albedo (Material.fs:68), SpecularTransmission -> 0 (:121) */
    int32_t nmat;      /* at most 65,536 (the path pool keeps a vertex's material in 16 bits) */
    int32_t width;     /* Film width  (Scene.fs:201-211) */
    int32_t height;    /* Film height */
    int32_t max_depth; /* PathIntegrator maxDepth; the reference hard-codes 3 (Scene.fs:304) */
    mfx_quad_light light;
    mfx_pinhole camera;
} mfx_scene_desc;

/* Context options.
 * Devices: with ndevices == 0 the context runs on `device`. With ndevices > 0 it drives
 * devices[0..ndevices) from this one process (the reference's in-process fan-out,
 * Integrators.fs:164, across GPUs) by an image partition: device g of G traces the film's
 * 8-pixel tile rows of band g of G — one of each G consecutive tile rows, at offset g in even groups
 * and G - 1 - g in odd ones (serpentine) — every sample of the context's sample partition, on its own
 * stream. Every per-pixel operation (the sample-order sum, Film.AddSample, the post) therefore runs
 * on one device in the one-device order, and every output is bit-identical to a one-device
 * context's. mfx_render_rgba8 (render-ahead included) copies each device's rows of the RGBA8
 * frame straight into the caller's buffer; mfx_sample and mfx_film_mean merge the devices' FP64
 * buffers on devices[0] (one RCCL reduce over a communicator the library owns, ncclCommInitAll over
 * the list; a pixel is +0.0 on every device but its own, so the sum is an exact merge). A list that
 * repeats a device (e.g. {0,0}) merges by device-ordered adds instead (RCCL needs distinct devices). */
typedef struct mfx_options {  /* ABI 4: the former `reserved` field is render_ahead (0 = off); layout unchanged since */
    uint64_t seed;      /* counter-RNG seed; the reference uses unseeded System.Random.
                         * All 64 bits enter every path's key; the key takes the global sample index
                         * modulo 2^32, so a pixel's sample streams repeat with period 2^32 */
    int32_t device;     /* HIP device ordinal when ndevices == 0 */
    int32_t flags;      /* MFX_F_* */
    int32_t part_index; /* this context renders sample partition part_index of part_count */
    int32_t part_count; /* (multi-process: one context per rank; partitions are disjoint sample sets;
                           with MFX_F_ROW_PARTITION disjoint sets of tile rows: band part_index of part_count) */
    int32_t ndevices;   /* 0: one device (`device`); 1..MFX_MAX_DEVICES: the device list below */
    int32_t render_ahead; /* 0 or 1: off. K in 2..MFX_MAX_RENDER_AHEAD: one-sample mfx_render_rgba8
                             calls (Scene.Render) take their sample from a batch of the next K
                             samples traced at once, on every device of a list (mfx_render_rgba8)  */
    const int32_t* devices; /* [ndevices] HIP device ordinals; devices[0] is the primary */
} mfx_options; /* 40 bytes */

#define MFX_F_NONE 0
#define MFX_F_COUNT_STATS 1 /* count traversal node/leaf/prim visits (slower; for the roofline model) */
#define MFX_F_MEGAKERNEL 2  /* one persistent megakernel instead of the wavefront pipeline */
#define MFX_F_HOST_BVH 4    /* build the traversal BVH on the host CPU (default: on the GPU; the same tree) */
#define MFX_F_WAVEFRONT 8   /* always the wavefront pipeline. Default: a call in which a device renders one
                               sample per pixel (Scene.Render) runs the megakernel, which is faster there
                               and gives the same bits (one path per pixel: no summation order) */
#define MFX_F_FLATTEN 16    /* mfx_create_instanced: flatten every instance into one BVH (no two-level
                               traversal); the same world scene, hits and images */
#define MFX_F_TWO_LEVEL 32  /* mfx_create_instanced: keep the two-level traversal. Default (neither flag):
                               flattened when the flat image fits MFX_FLATTEN_MAX_BYTES (env; default
                               2 GiB at 512 B per traversal slot of the expansion) and a sixteenth of
                               the device's free memory, two-level otherwise. Both flags: MFX_E_INVALID */
#define MFX_F_ROW_PARTITION 64 /* part_index / part_count partition the film's 8-pixel tile rows (serpentine
                               band part_index of part_count, as a device list's devices) instead of the
                               samples: a rank traces every sample of its rows,
                               its accumulator is +0.0 elsewhere, and a sum-reduce over the ranks is an exact
                               merge (the multi-process image partition; mfx_trace_accumulate)       */
#define MFX_F_IN_FLIGHT 128 /* the caller keeps frames in flight on several contexts of this device (each its
                               own pool and stream, frames alternating): the wavefront launches fetch larger
                               chunks of paths, since another frame's launches fill each launch's tail.
                               Scheduling only: the same images and ray counts (ABI 6, additive)     */

/* One entry of an instanced scene (mfx_create_instanced; an extension: the reference has no
 * instancing, its scenes are flat lists). The world primitive list — the index space Bvh.Build
 * sorts (BvhNode.fs:25) and every result refers to — is the concatenation, in entry order, of
 * each entry's copy of template primitives prims[first .. first + count): translated by `offset`
 * (every vertex, or a sphere's centre, + offset: one FP64 rounding per coordinate), or copied as
 * they are with MFX_INSTANCE_VERBATIM. Translated entries that share one template range are traced
 * through one template BVH (two-level traversal); everything else is flattened into the top level.
 * Results equal those of mfx_create on the expanded list (mfx_expand_instances), bit for bit.   */
typedef struct mfx_instance {
    int64_t first;
    int64_t count;
    double offset[3];
    int32_t flags;    /* MFX_INSTANCE_* */
    int32_t reserved;
} mfx_instance; /* 48 bytes */

#define MFX_INSTANCE_VERBATIM 1

typedef struct mfx_ctx mfx_ctx;

/* ---- lifetime ------------------------------------------------------------------------- */

/* Replaces `new Scene(state)` (Scene.fs:298-313): builds the reference's heap BVH leaf grouping
 * (BvhNode.fs:24-61), the GPU traversal BVH over it, uploads everything to HBM.
 * MFX_E_INVALID (before any BVH is built, on the host): a NaN or +-inf in what a primitive's kind reads
 * (a triangle's three corners, a rect's four, a sphere's centre and p[1][0]; the rest of p is not looked
 * at), in the light or in the camera (as mfx_set_camera: direction, fov and aspect count with
 * derived == 0, topleft, right and down otherwise); coordinates whose magnitude plus a ray's length
 * exceeds 2^126 (DESIGN.md §3 "Coordinate range"). The message names the first offender.          */
int mfx_create(const mfx_scene_desc* scene, const mfx_options* opt, mfx_ctx** out);
void mfx_destroy(mfx_ctx* ctx);
/* mfx_create for an instanced scene: scene->prims are the template primitives, `instances`
 * lists the entries whose expansion is the world scene (see mfx_instance).                    */
int mfx_create_instanced(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                         const mfx_options* opt, mfx_ctx** out);
/* Host-only: the world primitive list an instanced scene stands for (the library's own
 * expansion). out may be NULL to query the count; *nout = world primitives.                  */
int mfx_expand_instances(const mfx_prim* prims, int64_t nprims, const mfx_instance* instances,
                         int32_t ninstances, mfx_prim* out, int64_t cap, int64_t* nout);
/* How a context traces instances: out[0] = instances traced two-level, out[1] = template BVHs,
 * out[2] = top-level BVH4 nodes, out[3] = template BVH4 nodes, out[4] = slots per run of the
 * templates (each traced instance has its own run of world slots), out[5] = top-level slots,
 * out[6] = world slots, out[7] = bytes of the traversal images (nodes, slots, instance table).
 * All 0 but [5..7] for a flat context.                                                         */
int mfx_instancing_info(mfx_ctx* ctx, double out[8]);
/* Host-only (no device needed): the same figures for a scene built on the host from an instanced
 * description (MFX_F_FLATTEN honoured), plus the traversal stack bound. Without a device it
 * applies MFX_FLATTEN_MAX_BYTES alone: mfx_create_instanced also caps the flat image at a
 * sixteenth of the device's free memory, so on a nearly full device a context may trace two-level
 * where this reports flat (mfx_instancing_info out[0] > 0 tells a context's actual choice; the
 * images are the same either way).                                                              */
int mfx_build_instanced_info(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                             int32_t flags, double out[8], int32_t* stack_entries);

/* ---- several area lights (ABI 6, additive; an extension: a reference `Scene` holds one light) ------
 * A context has lights L_0 .. L_{N-1}, 1 <= N <= MFX_MAX_LIGHTS. Per light, creation computes the two
 * sample triangles, `area` and 1 / area exactly as for the one light of mfx_create, and then stores
 * pdf_n = (1.0 / area_n) / (double)N: two divisions, in that order.
 * At a path vertex (PathIntegrator.TraceRay, Integrators.fs:118-136):
 *  1. the hemisphere sample: unchanged, draw for draw;
 *  2. the pick, only when N >= 2: one more draw r, n = (int)floor(r * (double)N). With N == 1 no draw is
 *     taken and n = 0;
 *  3. light n's Sample_Li: the draws sel, tu, tv, then toLight, dist and the shadow query on
 *     [1e-6, dist - 1e-6];
 *  4. the direct term l = (unit . normal_hit) * L_n(toLight), with light n's normal, area and intensity:
 *     black unless toLight . normal_n < 0;
 *  5. the term added is l / pdf_n; in the kernels' factored form a_v = (cs * (solid_n * I_n[c])) / pdf_n,
 *     one rounding per operation;
 *  6. everything else (col, the fold (a_v + f) * c_v, depth handling, ray counts) is as with one light.
 * The pick is the reference's RandomDirectLightIntegrator (Integrators.fs:57-78: n = int(floor(
 * rand.NextDouble() * float lights.Length)), then SingleDirectLightIntegrator on lights[n]), with one
 * deliberate departure: the division by N inside pdf_n. The reference returns the picked light's own
 * pdf and so renders the mean of the lights; radiance is linear in emission, so the lights' sum is what
 * a scene with N lamps looks like, and that is what this renders (unbiased for the sum).
 * The pick needs no clamp: a draw is k * 2^-53 with k < 2^53, and (1 - 2^-53) * N rounds to a double
 * below N for every N <= MFX_MAX_LIGHTS (mafrixraytracing_amd/lights.py `pick` has the argument).
 * N == 1 through this entry point is, bit for bit, mfx_create (or mfx_create_instanced) with that light:
 * the same kernel instances, pool layout and grids.
 *
 * lights[0..nlights) replace scene->light, which is not read. instances == NULL && ninstances == 0 is
 * a flat scene; otherwise the call behaves as mfx_create_instanced. MFX_E_INVALID, decided on the host
 * before any device is touched: nlights < 1 or > MFX_MAX_LIGHTS, or NULL lights; a non-finite corner,
 * normal or intensity of a light (the message names the light's index and the field); with nlights >= 2
 * a light whose area is 0 or not finite (one light keeps mfx_create's behaviour), and MFX_F_MEGAKERNEL
 * or MFX_F_COUNT_STATS (the megakernel and the counting instances are built for one light only).
 * With N >= 2 every trace runs the wavefront pipeline, as under MFX_F_WAVEFRONT, and the pool keeps one
 * more byte per path vertex (the picked light of a lit vertex). Every sampling call composes with it
 * (the one-sample call, render-ahead, adaptive sampling and its resume, device lists, partitions,
 * mfx_set_camera); mfx_launch_info's out[13] (gray light) is 0.                                   */
int mfx_create_lights(const mfx_scene_desc* scene, const mfx_quad_light* lights, int32_t nlights,
                      const mfx_instance* instances, int32_t ninstances, const mfx_options* opt, mfx_ctx** out);
/* out[0] = N, out[1] = 1 if the several-light kernel instances run (N >= 2), out[2] = bytes of the
 * device light table, out[3] = bytes per path slot the lights add to the pool (0 with one light),
 * out[4] / out[5] = resident blocks per CU of the k_shadow / k_resolve instance in use, the rest 0.  */
int mfx_light_info(mfx_ctx* ctx, double out[8]);
/* Host-only (no device needed): what creation derives from the lights, by the code creation runs.
 * out[nlights][4] = area, 1 / area, pdf_n, 0. The same refusals as mfx_create_lights' for the lights. */
int mfx_light_table(const mfx_quad_light* lights, int32_t nlights, double* out);

/* ---- albedo textures (ABI 6, additive; an extension: the reference's materials are one colour each) ------
 * A primitive may carry a UV map and a texture; at every path vertex on it the material's albedo is
 * multiplied by one texel, looked up by the nearest-texel rule below. A lookup is an exact table read and
 * the only arithmetic is the texel's index, stated in + - * / floor, so a host statement
 * (mafrixraytracing_amd/textures.py) and the kernels agree bit for bit. Every material stays Lambertian.
 * All FP64, one rounding per operation, no contraction; dot(a,b) = (a0*b0 + a1*b1) + a2*b2.
 *
 * Inputs. mfx_texture: `rgba` is width * height texels of 4 bytes, rows top to bottom; alpha is ignored and
 * the bytes are taken as linear (a caller who wants sRGB decodes before the call). mfx_prim_uv: one per
 * entry of scene->prims; texture == -1: the primitive is untextured; uv[i] belongs to corner p[i]. A rect
 * uses the map of its first three corners for the whole rect (exact for a parallelogram with an affine
 * layout, which is what OBJ quads are). A sphere must have texture == -1.
 *
 * The UV record. Each *world* primitive (after instance expansion: the template's corners plus the offset, so
 * every instance has its own records) gets 8 doubles, computed on the host at creation from its world corners
 * v0, v1, v2:
 *  1. e1 = v1 - v0, e2 = v2 - v0;
 *  2. d11 = dot(e1,e1), d12 = dot(e1,e2), d22 = dot(e2,e2);
 *  3. det = d11*d22 - d12*d12;
 *  4. for w in (u, v), with w0, w1, w2 the corners' coordinates: dw1 = w1 - w0, dw2 = w2 - w0;
 *     a = (d22*dw1 - d12*dw2)/det; b = (d11*dw2 - d12*dw1)/det; g[c] = e1[c]*a + e2[c]*b;
 *     cw = w0 - dot(v0, g);
 *  5. the record is gu[3], cu, gv[3], cv;
 *  6. if det == 0, or any of the eight values is not finite, the record is 0,0,0,u0, 0,0,0,v0: a degenerate
 *     primitive shows the texel of its first corner.
 * At a path vertex, hp being the hit point that starts the shadow ray, on a primitive with a W x H texture:
 *     u = dot(hp, gu) + cu, v = dot(hp, gv) + cv;
 *     tu = u - floor(u); xi = (int)floor(tu * (double)W) clamped into [0, W-1] (tu is exactly 1.0 for a tiny
 *     negative u); yi likewise with tv and H; row = (H-1) - yi (OBJ's v points up);
 *     id = base_t + row*W + xi, base_t being the texture's offset in the concatenation of all textures' texels.
 * The albedo at that vertex: a[c] = albedo[mat][c] * ((double)texel[id][c] / 255.0); on an untextured primitive
 * albedo[mat][c] as ever. A 255 byte gives a factor of exactly 1.0: an all-white texture changes no bit.
 * Everything else of the vertex is unchanged. mfx_aov's planes [4..6] take the same a at the first hit;
 * mfx_denoise, mfx_denoise_var and mfx_temporal run unchanged on those features.                          */
typedef struct mfx_texture {
    const uint8_t* rgba;
    int32_t width, height; /* 1 .. 16384 each */
} mfx_texture; /* 16 bytes */
typedef struct mfx_prim_uv {
    int32_t texture;  /* index into `textures`, or -1 */
    int32_t reserved;
    double uv[3][2];  /* (u, v) of p[0], p[1], p[2] */
} mfx_prim_uv; /* 56 bytes */
#define MFX_MAX_TEXTURES 4096
#define MFX_MAX_TEXTURE_DIM 16384

/* mfx_create_lights with textures: lights and instances exactly as there; prim_uv[scene->nprims].
 * ntextures == 0, or every texture == -1, is bit for bit and kernel for kernel the call without textures: the
 * same mfx_launch_info, pool bytes and mfx_build_info digest (the UV table and the texels are arrays of their
 * own; the digest does not cover them). Otherwise the context runs the textured instances of k_shadow,
 * k_resolve and mfx_aov's kernel, always the wavefront pipeline (one-sample calls included), and its path
 * pool keeps 4 bytes more per path vertex: the vertex's texel id. The texels are copied to the device at
 * creation and stay there across an mfx_set_camera rebuild (the records depend on the primitives alone).
 * MFX_E_INVALID, decided on the host before any device is touched, the message naming the first offender:
 * ntextures < 0 or > MFX_MAX_TEXTURES, or NULL textures with ntextures > 0; a width or height outside
 * [1, MFX_MAX_TEXTURE_DIM]; more than 2^31 - 2 texels in all (these three from the sizes alone, before any
 * texel or pointer is looked at); a NULL rgba; NULL prim_uv with ntextures > 0; a texture index outside
 * [-1, ntextures); a textured sphere; a non-finite uv of a textured primitive; with any textured primitive,
 * MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS (those kernel instances are built without textures).             */
int mfx_create_textured(const mfx_scene_desc* scene, const mfx_quad_light* lights, int32_t nlights,
                        const mfx_instance* instances, int32_t ninstances, const mfx_texture* textures,
                        int32_t ntextures, const mfx_prim_uv* prim_uv, const mfx_options* opt, mfx_ctx** out);
/* out[0] = textures, out[1] = 1 if the textured kernel instances run, out[2] = bytes of texels on the device,
 * out[3] = bytes of the UV table (64 per world primitive, plus 4 for its texture index), out[4] = bytes per
 * path slot the textures add to the pool, out[5] / out[6] = resident blocks per CU of the k_shadow /
 * k_resolve instance in use, out[7] = 0. A context without textured primitives reports 0 in [0..4].        */
int mfx_texture_info(mfx_ctx* ctx, double out[8]);
/* Host-only (no device needed): the UV records of prims[0..nprims) as given (no instance expansion), by the
 * code creation runs; out[nprims][8]. A primitive with texture == -1, or a sphere, gets eight zeros.       */
int mfx_uv_table(const mfx_prim* prims, int64_t nprims, const mfx_prim_uv* prim_uv, double* out);
/* Host-only: the texel rule. id_out[k] = the id of uv[k] in texture `texture` of the concatenation of
 * textures[0..ntextures) (only the sizes are read: rgba may be anything). MFX_E_INVALID: the size refusals
 * of mfx_create_textured, or a texture index outside [0, ntextures).                                       */
int mfx_texel_index(const mfx_texture* textures, int32_t ntextures, int32_t texture, int64_t n, const double* uv,
                    uint32_t* id_out);

/* ---- the camera (an extension of the ABI: the reference's PinholeCamera has mutable position /
 * topleft / coord, Camera.fs:122-133, and Film.Reset exists for a camera move). Additive in ABI 6. ---- */

/* Host-only (no device needed): the constructor mfx_create runs on mfx_scene_desc.camera (with
 * derived != 0 the fields as they are). out = position, topleft, right, down (3 doubles each).
 * MFX_E_INVALID: a NULL argument.                                                              */
int mfx_pinhole_derive(const mfx_pinhole* cam, double out[12]);
/* out[0..11] = the context's current derived camera (position, topleft, right, down), out[12] = the
 * camera epoch: 0 after create, +1 per mfx_set_camera that changed the camera, out[13] = the widening
 * eps the traversal images were built with, out[14] = the eps the current camera needs
 * ((float)ldexp(R + T, -19), DESIGN.md §3: out[14] <= out[13] always), out[15] = the number of times
 * mfx_set_camera had to build the images again.                                                 */
int mfx_camera_info(mfx_ctx* ctx, double out[16]);
/* Makes `cam` the camera of every later call, on every device of a device list. Waits for the
 * context's work first, a render-ahead batch traced in the background included.
 * In place: when the widening the new position needs is at most the one the images were built with
 * (two-level scenes: the template BVHs' too), only the camera changes: the boxes stay conservative
 * for every ray the new camera starts, and every result is what a context created with `cam` gives.
 * Rebuild: otherwise the scene is prepared again for the new camera from the description the context
 * has kept since creation (host memory: 104 B per primitive, plus the material and instance tables),
 * by mfx_create's own code: afterwards mfx_build_info's digest, the launch shapes and every result
 * are those of a fresh mfx_create with `cam` (an instanced scene keeps the flat / two-level choice of
 * its creation). The seed, the options, next_sample, the film and its frame count and the
 * accumulator's contents are kept. A failed rebuild leaves the old camera and images in place and
 * returns the error.
 * What it invalidates: frames held by render-ahead are never served afterwards (the next one-sample
 * call traces a new batch from the film as it then is); an adaptive result (mfx_sample_adaptive_resume
 * and MFX_DN_SRC_ADAPTIVE return MFX_E_STATE until mfx_sample_adaptive runs again: a resume must not
 * mix cameras); the feature buffers (mfx_denoise, mfx_denoise_var and mfx_temporal return MFX_E_STATE
 * until mfx_aov runs again). The temporal history is kept: mfx_temporal reprojects it.
 * What it leaves alone: the film, the accumulator, next_sample and the ray counters. As in the
 * reference, where moving the camera and Film.Reset are separate, the caller decides whether the film
 * starts over: call mfx_reset (and mfx_accum_clear) after the move, or the film mixes both views.
 * A camera whose derived fields are bit-equal to the current ones is a successful no-op: no wait, no
 * new epoch. MFX_E_INVALID: a NULL argument, a non-finite field (direction, fov and aspect count only
 * with derived == 0, topleft, right and down only with derived != 0) or a non-finite derived camera,
 * a zero direction with derived == 0.                                                           */
int mfx_set_camera(mfx_ctx* ctx, const mfx_pinhole* cam);

/* ---- the sky (ABI 6, additive; an extension: in the reference a ray that leaves the scene returns black,
 * TraceRay's `else Color()`, Integrators.fs:137) ---------------------------------------------------------
 * The environment is a square octahedral map of size x size texels, 1 <= size <= MFX_MAX_ENV_SIZE (at most
 * 2^24 texels: a texel id fits in 24 bits). A texel is three floats, linear RGB radiance, widened to double
 * exactly: E[c] = (double)rgb[3*id + c]. size == 1 is a constant sky. No trigonometry: the texel of a
 * direction is stated in + - * / abs floor and comparisons, so a host statement
 * (mafrixraytracing_amd/environment.py) and the kernels agree bit for bit, as for mfx_texel_index.
 *
 * The texel of a direction. d is the ray's unit direction as the kernels hold it; all FP64, one rounding per
 * operation, no contraction; +y is the pole (the camera's up):
 *  1. s = (|dx| + |dy|) + |dz|; px = dx / s; pz = dz / s;
 *  2. if dy >= 0.0 (which includes -0.0): a = px, b = pz;
 *  3. otherwise a = (1.0 - |pz|) * sg(px), b = (1.0 - |px|) * sg(pz), with sg(x) = x >= 0.0 ? 1.0 : -1.0;
 *  4. u = a * 0.5 + 0.5; v = b * 0.5 + 0.5;
 *  5. xi = (int)floor(u * (double)size) clamped into [0, size-1]; yi likewise from v;
 *  6. id = yi * size + xi.
 *
 * The estimator is the reference's with one change: TraceRay(ray, depth) for depth >= 0 returns E(ray.direction)
 * on a miss instead of Color(); a hit is handled as ever. The depth -1 query stays untraced and black. So the
 * rays traced, the iterations and every ray counter are those of the same context without an environment. A
 * path whose ray missed after nv vertices folds f = E, then f <- (a_v + f) * c_v for v = nv-1 .. 0, over all
 * nv vertices, the unlit ones included; a camera ray that misses (nv = 0) contributes E itself, so the
 * background shows; a path that ends by depth alone is as without. Shadow rays ignore the sky, and the sky is
 * not light-sampled: only the hemisphere-sampled extension ray sees it, no draw is added and the RNG stream is
 * unchanged. A small bright sun in the map will therefore be noisy (mfx_set_environment_sampled below samples
 * the map as a light instead). Every surface stays Lambertian, so
 * mfx_temporal's view independence holds, and mfx_aov's first-hit planes do not depend on the sky (a miss
 * still adds nothing there).                                                                             */
typedef struct mfx_environment {
    const float* rgb; /* size * size texels of 3 floats, row yi after row yi-1 */
    int32_t size;     /* 1 .. MFX_MAX_ENV_SIZE */
    int32_t reserved;
} mfx_environment; /* 16 bytes */
#define MFX_MAX_ENV_SIZE 4096

/* Makes `env` the sky of every later call, on every device of a device list (the texels are copied to each);
 * env == NULL removes it, and the context is then the one it was before, kernel for kernel: the same
 * mfx_launch_info, pool bytes and images. It composes with every creation entry point: it touches no BVH,
 * slot or digest. With an environment the context runs the ENV instances of k_extend, k_camera and k_resolve,
 * always the wavefront pipeline (one-sample calls included), and its path pool keeps 4 bytes more per slot:
 * the miss record. Waits for the context's work first, a render-ahead batch traced in the background included.
 * What it invalidates: what mfx_set_camera invalidates, except the feature buffers (they do not depend on
 * the sky): frames held by render-ahead are never served afterwards, and an adaptive result is gone
 * (mfx_sample_adaptive_resume and MFX_DN_SRC_ADAPTIVE return MFX_E_STATE until mfx_sample_adaptive runs
 * again). What it leaves alone: the film, the accumulator, next_sample, the ray counters, the feature buffers
 * and the temporal history. An mfx_set_camera rebuild keeps the environment.
 * MFX_E_INVALID, decided on the host, the message naming the first offender: a size outside
 * [1, MFX_MAX_ENV_SIZE]; a NULL rgb (both only with a non-NULL env); a texel that is not finite or is
 * negative. MFX_E_STATE: a context created with MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS (those kernel
 * instances are built without an environment).                                                            */
int mfx_set_environment(mfx_ctx* ctx, const mfx_environment* env);
/* out[0] = size, out[1] = 1 if the environment instances run, out[2] = bytes of texels on the device,
 * out[3] = bytes per path slot the environment adds to the pool, out[4] / out[5] = resident blocks per CU of
 * the k_extend / k_resolve instance in use, out[6] = out[7] = 0. All 0 without an environment.            */
int mfx_environment_info(mfx_ctx* ctx, double out[8]);
/* Host-only (no device needed): the texel rule, by the code the kernels compile. id_out[k] = the texel of
 * direction dirs[3k .. 3k+2] in a size x size map. MFX_E_INVALID: a size outside [1, MFX_MAX_ENV_SIZE], a
 * NULL array with n > 0, n < 0.                                                                           */
int mfx_env_texel_index(int32_t size, int64_t n, const double* dirs, uint32_t* id_out);

/* ---- the sky as a light (ABI 6, additive; an extension like the sky itself) -------------------------------
 * mfx_set_environment_sampled is mfx_set_environment, and the sky becomes the (N+1)-th light of the pick of
 * mfx_create_lights: it is sampled at every path vertex in proportion to its radiance, so a small bright sun
 * in the map is found by one vertex in N + 1 instead of one in 1e5. N >= 1 is the number of area lights, at
 * most MFX_MAX_SKY_LIGHTS: the sky takes light index N.
 *
 * Everything is FP64 with one rounding per operation in the order written and no contraction.
 * dot(a,b) = (a0*b0 + a1*b1) + a2*b2, sg(x) = x >= 0.0 ? 1.0 : -1.0, INVPI = 1. / 3.141592653589793.
 *
 * The table, built on the host when the sky is set; n = size*size:
 *  - the weight of texel t is w_t = ((r + g) + b) * (1.0 / (len2_c * len_c)), r, g, b the texel widened
 *    exactly, len2_c and len_c from the direction rule below at the texel's centre (ju = jv = 0.5): the
 *    sampling density per solid angle is proportional to the texel's radiance. If every w_t is 0 (a black map)
 *    every w_t is 1.0;
 *  - an alias table over the w_t (Vose's method; the construction is the library's, deterministic for a given
 *    map): per texel a float q[k] in [0, 1] and a uint32 alias[k];
 *  - per texel the probability those two arrays imply, an exact statement of the arrays:
 *    prob[t] = (q_t + sum over k with alias[k] == t, k != t, of (1 - q_k)) / n, q widened to double exactly,
 *    the sum taken in increasing k from (double)q_t;
 *  - a texel with w_t = 0 has q = 0 and is no entry's alias, so it is never returned.
 *
 * At a path vertex the steps are mfx_create_lights' steps 1-6 with N + 1 in place of N everywhere:
 *  - the pick draw is taken always (N + 1 >= 2): n = (int)floor(r * (double)(N + 1));
 *  - for n < N the vertex is an area-light vertex exactly as there, with pdf_n = (1.0 / area_n) / (double)(N + 1);
 *  - for n == N, the sky:
 *    1. four more draws, in this order: r1, r2, ju, jv;
 *    2. k = (int)floor(r1 * (double)n_texels) clamped into [0, n_texels - 1]; t = r2 < (double)q[k] ? k : alias[k];
 *       xi = t % size, yi = t / size;
 *    3. the direction of (t, ju, jv): u = ((double)xi + ju) / (double)size, a = u * 2.0 - 1.0; b likewise from
 *       yi, jv; py = (1.0 - |a|) - |b|; if (|a| + |b|) <= 1.0 then px = a, pz = b, otherwise
 *       px = (1.0 - |b|) * sg(a), pz = (1.0 - |a|) * sg(b); len2 = (px*px + py*py) + pz*pz, len = sqrt(len2),
 *       unit = (px/len, py/len, pz/len). This is the inverse of the texel rule above. The radiance used is
 *       texel t's, by id, not a second lookup of unit;
 *    4. cs = dot(unit, nm); the vertex is lightable iff cs > 0.0: the sky lights the side the normal points
 *       to, the side the extension ray sees it from;
 *    5. pdf_v = (((prob[t] * (double)(size*size)) * 0.25) * (len2 * len)) / (double)(N + 1) (a texel covers
 *       4/size^2 of the (a, b) square, and d omega = da db / len^3);
 *    6. the shadow query is the any-hit of Ray(hp, unit) on [1e-6, 99999999.], the extension ray's far bound;
 *    7. the vertex is lit iff it is lightable and not occluded; its direct term is
 *       a_v[c] = ((cs * E_t[c]) * INVPI) / pdf_v. (The INVPI is there because the fold multiplies the direct
 *       term by col = 2 a ei, whose mean is the albedo; the reference's area-light term carries no 1/pi, a
 *       radiance map needs it.)
 *  - the fold f <- (a_v + f) * c_v, the hemisphere sample and the ray counters are as ever: one shadow ray per
 *    vertex, and the primary, extension and shadow counts are those of the same context under a black sampled
 *    sky. (Against a context with no sky they are equal where they do not depend on the draws: the pick draw and
 *    the sky vertex's fifth draw move the later hemisphere samples to other draws, so in an open scene a path may
 *    leave at another vertex.)
 *
 * The miss term under sampling: a camera ray that misses (nv = 0) still returns E, so the background shows; a
 * later miss returns black, since the sky now reaches surfaces through the pick alone and would be counted
 * twice. Consequence: a sampled sky lights every vertex 0 .. max_depth, as the area lights do, where an
 * unsampled sky lights 0 .. max_depth - 1 (the last vertex sends no extension ray). With all light intensities
 * 0, the sampled sky at depth D and the unsampled sky at depth D + 1 have the same expectation.
 *
 * The context runs the SKY instances of k_shadow and k_resolve (twins of the several-light ones, so one area
 * light beside a sampled sky runs several-light instances and mfx_light_info reports them), the ENV instances
 * of k_camera / k_extend for the camera rays and the plain ones for the bounces. The pool keeps 4 bytes more
 * per path vertex (a sky vertex's texel id), and with one area light the byte per vertex of the light index.
 * Out of scope: multiple importance sampling with the hemisphere sample, a power-proportional pick.        */
#define MFX_MAX_SKY_LIGHTS 63   /* area lights at most beside a sampled sky: the sky takes light index N */

/* mfx_set_environment, and the sky becomes a light that is sampled at every path vertex (the rule above).
 * env == NULL removes the sky, as there. mfx_set_environment(ctx, env) on such a context makes the sky an
 * unsampled one again. Refusals: mfx_set_environment's; MFX_E_STATE also for a context with 64 lights (the
 * message names the count). A refused call changes nothing. It invalidates and keeps what mfx_set_environment
 * does; a switch between none, unsampled and sampled releases the path pool (its layout changes), and the
 * lights' pdf_n is recomputed with N + 1 when sampling goes on and with N when it goes off. An mfx_set_camera
 * rebuild keeps the sampling. */
int mfx_set_environment_sampled(mfx_ctx* ctx, const mfx_environment* env);
/* out[0] = 1 if the sky is sampled, out[1] = N + 1, out[2] = bytes of the sampling table on the device
 * (16 per texel), out[3] = bytes per path slot it adds to the pool (4 per vertex, 5 with one area light),
 * out[4] / out[5] = resident blocks per CU of the k_shadow / k_resolve instance in use, out[6] = out[7] = 0.
 * All 0 otherwise. */
int mfx_sky_sampling_info(mfx_ctx* ctx, double out[8]);
/* Host-only: the table creation builds from a map, by the code creation runs. q[n], alias[n], prob[n],
 * n = size * size. The refusals of mfx_set_environment for the map. */
int mfx_env_sample_table(const mfx_environment* env, float* q, uint32_t* alias, double* prob);
/* Host-only: the direction rule, by the code the kernels compile. For texel[k] and jitter[2k], jitter[2k+1]:
 * out[4k .. 4k+2] = the unit direction, out[4k+3] = len2 * len (the Jacobian factor of the pdf).
 * MFX_E_INVALID: a size outside [1, MFX_MAX_ENV_SIZE], a texel outside the map, a NULL array with n > 0, n < 0. */
int mfx_env_sample_direction(int32_t size, int64_t n, const uint32_t* texel, const double* jitter, double* out);

/* ---- the thin lens (ABI 6, additive; an extension: the reference's camera is PinholeCamera alone) ---------
 * While a lens is set, every camera ray starts from a point of a disk around the camera position and passes
 * through the point where the pinhole ray of the same (u, v) meets the focus plane: what lies in that plane is
 * sharp, the rest is blurred by the disk. aperture is the lens radius in world units, focus the distance of the
 * plane of sharp focus along the forward axis.
 *
 * Everything is FP64 with one rounding per operation in the order written and no contraction.
 * dot(a,b) = (a0*b0 + a1*b1) + a2*b2.
 *
 * The lens record, on the host, when the lens is set or the camera changes. P0, TL, R, D are the derived
 * camera's position, topleft, right and down (mfx_pinhole_derive):
 *  1. lr = sqrt(dot(R,R)); ld = sqrt(dot(D,D));
 *  2. U[c] = (R[c] / lr) * aperture; V[c] = (D[c] / ld) * aperture;
 *  3. n = cross(R, D): n0 = R1*D2 - R2*D1, n1 = R2*D0 - R0*D2, n2 = R0*D1 - R1*D0;
 *  4. ln = sqrt(dot(n,n)); f[c] = n[c] / ln, the forward axis (the constructor's direction, normalised);
 *  5. dplane = dot(TL - P0, f) (0.5 for a constructed camera, up to rounding);
 *  6. s = focus / dplane;
 *  7. the record is U[3], V[3], s: seven doubles.
 *
 * A camera ray. Pixel, sample, key and u, v are as ever (the path's first two draws):
 *  1. target = (TL + R*u) + D*v, the pinhole's expression; pin = target - P0;
 *  2. the lens point comes from a stream of its own, so the path's stream does not move: draw m is
 *     rng_unit(mix64(key + m * 0x9e3779b97f4a7c15)), as rng_next with counter m, and the lens uses counters
 *     2^31 + 1, 2^31 + 2, ... of the path's own key. The path's counter goes on at 2 (a path's own counter
 *     stays far below 2^31);
 *  3. per trial: r1, r2 are the next two lens draws; a = r1*2.0 - 1.0; b = r2*2.0 - 1.0; the trial is accepted
 *     iff (a*a + b*b) < 1.0 (rejection, as the reference's GetRandomInUnitSphere: no trigonometry);
 *  4. o = (P0 + U*a) + V*b;
 *  5. fp = P0 + pin*s;
 *  6. d = normalize(fp - o), the camera ray's own normalisation (x / l, l = sqrt(x*x + y*y + z*z), 0 for l == 0);
 *  7. Ray(o, d) is traced on [1e-6, 99999999.], as a camera ray is.
 * Everything after the first hit is unchanged; under a sky a camera ray's miss records the texel of d.
 * mfx_aov traces these rays too: its planes are the film's own rays', and plane [3] is t along the lens ray.  */
typedef struct mfx_lens {
    double aperture; /* the lens radius, world units; finite, >= 0; exactly 0: no lens */
    double focus;    /* the distance of the focus plane along the forward axis; finite, > 0 */
} mfx_lens; /* 16 bytes */

/* Makes `lens` the lens of every later call, on every device of a device list; NULL, or an aperture of exactly
 * 0, removes it, and the context is then the pinhole one again, kernel for kernel: the same mfx_launch_info,
 * pool bytes, digest and images. It composes with every creation entry point and every sampling call. With a
 * lens the context runs the LENS twin of the k_extend instance that starts a generation's paths (flat scenes
 * too: no camera packets and no camera cuts, which rest on one shared origin) and of k_aov, and always the
 * wavefront pipeline (one-sample calls included); k_shadow, k_resolve, the bounces and the pool are as without.
 * Waits for the context's work first, as mfx_set_camera does.
 * The widening: the traversal boxes' eps is sized by the magnitudes of ray origins, and lens origins lie off P0
 * by up to |U| + |V| per axis. The eps needed is the largest over the eight corners of that box; if the images'
 * eps covers it only the lens changes, otherwise the images are built again by creation's code for that corner
 * (a failed rebuild leaves the old state in place). Images built for a lens are built again for the camera alone
 * when the lens is removed. mfx_set_camera under a lens keeps aperture and focus, derives the record again and
 * applies the same rule.
 * What it invalidates: what mfx_set_camera invalidates (held render-ahead frames, the adaptive result, the
 * feature buffers). What it leaves alone: the film, the accumulator, next_sample, the ray counters, the sky,
 * the lights and the textures. mfx_temporal returns MFX_E_STATE under a lens (its reprojection is the
 * pinhole's) and leaves the history as it is; mfx_denoise and mfx_denoise_var run unchanged on the lens features.
 * MFX_E_INVALID, decided on the host before a device is touched, the message naming the field: an aperture
 * that is not finite or negative; a focus that is not finite or not > 0; a camera for which lr, ld, ln or
 * dplane is zero or not finite, or dplane <= 0; a non-finite s. MFX_E_STATE: a context created with
 * MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS. A refused call changes nothing.                                  */
int mfx_set_lens(mfx_ctx* ctx, const mfx_lens* lens);
/* out[0] = 1 with a lens, out[1] = aperture, out[2] = focus, out[3..5] = U, out[6..8] = V, out[9] = s,
 * out[10] = the eps the lens camera needs, out[11] = the image rebuilds mfx_set_lens caused, out[12] / out[13] =
 * resident blocks per CU of the k_extend instance that starts the paths / of the k_aov instance in use, the
 * rest 0. All 0 without a lens.                                                                          */
int mfx_lens_info(mfx_ctx* ctx, double out[16]);
/* Host-only (no device needed), by the code the kernels compile: the record of `cam` under `lens`,
 * out = U[3], V[3], s. The MFX_E_INVALID refusals of mfx_set_lens (an aperture of 0 is accepted: U = V = 0). */
int mfx_lens_derive(const mfx_pinhole* cam, const mfx_lens* lens, double out[7]);
/* Host-only: the camera rays of n paths, path i being sample sample[i] of pixel (px[i], py[i]) of a
 * width x height film under `seed`: out[8i .. 8i+7] = o, d, a, b and trials[i] = the rejection trials it took.
 * MFX_E_INVALID: mfx_lens_derive's refusals, a film size below 1, a pixel outside the film, a negative sample,
 * n < 0, a NULL array with n > 0.                                                                        */
int mfx_lens_rays(const mfx_pinhole* cam, const mfx_lens* lens, uint64_t seed, int32_t width, int32_t height, int64_t n,
                  const int32_t* px, const int32_t* py, const int64_t* sample, double* out, int32_t* trials);

/* ---- smooth shading (ABI 6, additive; an extension: the reference shades every triangle and rect with its
 * face normal, Triangle.normal, and keeps the interpolation of corner normals commented out) ---------------
 * A triangle or rect may carry a normal per corner; at every path vertex on it, and at mfx_aov's first hit,
 * the interpolated normal replaces the face normal as the shading normal. All FP64, one rounding per operation
 * in the order written, no contraction, + - * / sqrt only; dot(a,b) = (a0*b0 + a1*b1) + a2*b2. A host statement
 * (mafrixraytracing_amd/normals.py) and the kernels agree bit for bit.
 *
 * Input. mfx_prim_normals: one per entry of scene->prims; smooth == 0: the primitive keeps its face normal;
 * n[i] belongs to corner p[i] and need not be unit length. A rect uses the affine map of its first three
 * corners for the whole rect, as mfx_prim_uv does. A sphere must have smooth == 0: it has its own normal.
 *
 * The normal record. Each *world* primitive (after instance expansion, so the result equals a flat create of
 * the expanded list) gets 12 doubles, computed on the host from its world corners v0, v1, v2:
 *  1. steps 1-3 of the UV record, unchanged: e1, e2, d11, d12, d22, det;
 *  2. for each component c in 0..2, with w_i = n[i][c]: dw1 = w1 - w0; dw2 = w2 - w0;
 *     a = (d22*dw1 - d12*dw2)/det; b = (d11*dw2 - d12*dw1)/det; g_c[k] = e1[k]*a + e2[k]*b;
 *     k_c = w0 - dot(v0, g_c);
 *  3. the record is g_0[3], k_0, g_1[3], k_1, g_2[3], k_2;
 *  4. if det == 0, or any of the twelve values is not finite, the record is 0,0,0,n[0][0], 0,0,0,n[0][1],
 *     0,0,0,n[0][2]: a degenerate primitive shows its first corner's normal.
 * At a path vertex on a smooth primitive, and at mfx_aov's first hit on one, hp being the stored hit point and
 * ng the normal the vertex has without this call:
 *  1. r[c] = dot(hp, g_c) + k_c;
 *  2. l = sqrt((r0*r0 + r1*r1) + r2*r2);
 *  3. if l is not finite or not > 0, ns = ng; otherwise ns = (r0/l, r1/l, r2/l);
 *  4. if dot(ns, ng) < 0.0, ns = (-ns0, -ns1, -ns2): the shading normal stays on the face normal's side
 *     whatever the winding convention of the caller's normals;
 *  5. ns replaces the vertex's normal for everything after it: the hemisphere sampler's rejection test, ei, cs,
 *     and mfx_aov's planes [0..2].
 * Nothing else moves: the hit point, the rays' origins, the order of the draws, the shadow query and the
 * unclamped cosine are as without. There is no terminator or light-leak correction: a sampled direction may
 * point below the geometric surface, and it is traced as it is. Every surface stays Lambertian and the shading
 * normal does not depend on the view, so mfx_temporal's argument holds unchanged.                          */
typedef struct mfx_prim_normals {
    int32_t smooth;    /* 0: the primitive keeps its face normal */
    int32_t reserved;
    double n[3][3];    /* normals of corners p[0], p[1], p[2]; need not be unit length */
} mfx_prim_normals; /* 80 bytes */

/* Makes pn[nprims] (nprims == the scene's template primitive count) the corner normals of every later call, on
 * every device of a device list (the tables are copied to each); NULL removes them, and the context is then the
 * one it was, kernel for kernel: the same mfx_launch_info, pool bytes, digest and images. It works on a context
 * from any creation entry point. With normals the context runs the SN twins of k_shadow and of k_aov, and always
 * the wavefront pipeline (one-sample calls included); a pn whose every smooth is 0 still runs them and changes no
 * bit. k_extend, k_camera, k_resolve and the pool are as without. Waits for the context's work first.
 * What it invalidates: what mfx_set_camera invalidates (held render-ahead frames, the adaptive result, the
 * feature buffers). What it leaves alone: the film, the accumulator, next_sample, the ray counters, the sky, the
 * lens, the lights, the textures and the temporal history. An mfx_set_camera or mfx_set_lens rebuild keeps the
 * normals: the records depend on the primitives alone.
 * MFX_E_INVALID, decided on the host before a device is touched, the message naming the first offender: nprims
 * differs from the context's template primitive count; a smooth sphere; a non-finite normal of a smooth
 * primitive. MFX_E_STATE: a context created with MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS. A refused call changes
 * nothing.                                                                                                 */
int mfx_set_normals(mfx_ctx* ctx, const mfx_prim_normals* pn, int64_t nprims);
/* out[0] = smooth world primitives, out[1] = 1 if the SN kernel instances run, out[2] = device bytes of the
 * tables (96 per world primitive plus 4 for its flag), out[3] = 0 (no pool bytes are added), out[4] / out[5] =
 * resident blocks per CU of the k_shadow / k_aov instance in use, the rest 0. All 0 without normals.       */
int mfx_normal_info(mfx_ctx* ctx, double out[8]);
/* Host-only (no device needed): the normal records of prims[0..nprims) as given (no instance expansion), by the
 * code mfx_set_normals runs; out[nprims][12]. A primitive with smooth == 0, or a sphere, gets twelve zeros. */
int mfx_normal_table(const mfx_prim* prims, int64_t nprims, const mfx_prim_normals* pn, double* out);
/* Host-only, by the code the kernels compile: out[k] = the shading normal at hit point hp[k] under record
 * rec[k] of a vertex whose normal is ng[k] (steps 1-4 above).                                              */
int mfx_shading_normal(int64_t n, const double* rec, const double* ng, const double* hp, double* out);

/* ---- the reference's render API --------------------------------------------------------- */

/* == IPixelIntegrator.Sample(spp) (IIntegrator.fs:35-40, Integrators.fs:161-172):
 * renders spp fresh samples per pixel and writes their mean as Color[w,h], x-major:
 * frame[(i*h + j)*4 + {0,1,2,3}] = r,g,b,1.0 for column i, row j (row 0 = top).
 * Successive calls draw successive global sample indices (the reference's RNG keeps
 * running between calls).                                                                  */
int mfx_sample(mfx_ctx* ctx, int32_t spp, double* frame_xmajor_rgba);

/* ---- adaptive sampling (an extension: the reference gives every pixel the same budget) ------
 * mfx_sample with a per-tile early stop. Additive in ABI 6.
 *
 * Tiles are the film's 8x8 pixel tiles: tiles_x = ceil(w/8), tiles_y = ceil(h/8), tile
 * T = ty * tiles_x + tx; a tile's valid pixels are those inside the film, m of them (1 <= m <= 64).
 * For one sample of pixel p let (fx, fy, fz) be the path's radiance (0 for a path with no lit
 * vertex) and Y = (fx + fy) + fz. Beside the accumulator the call keeps two FP64 planes,
 * S1_p = sum Y and S2_p = sum Y*Y, summed in sample order, FP64, no contraction. After n samples
 * of every pixel of a tile:
 *     v_p = max(0, S2_p - S1_p*S1_p/n) / (n*(n-1))        (variance of the pixel's mean)
 *     E = sum over valid p of v_p,   M = sum over valid p of S1_p/n
 *     converged  <=>  E*m <= rel_error^2 * (|M| + abs_floor*m)^2
 * i.e. the RMS standard error of the tile's pixels is at most rel_error x (the magnitude of the
 * tile's mean luminance + abs_floor); |M| because the reference's cosine is unclamped and radiance
 * can be negative. A black tile has E = 0 and converges at the first check.
 * Schedule: every tile gets min_spp samples and is checked; an unconverged tile gets step_spp more
 * (clipped so that it never exceeds max_spp) and is checked again; a tile stops at the first check
 * it passes, or at max_spp. All tiles still active have had the same number of samples: one pass
 * is one sample range over the list of active tiles.
 * Samples: a tile that stops at n uses global samples [next_sample, next_sample + n), next_sample
 * being the running counter mfx_sample advances; the call then advances it by max_spp whatever
 * the tiles did, so later calls draw samples no pixel has used. A pixel's value is, bit for bit,
 * the sum in sample order of its samples 0..n-1 divided by n (color / float n).
 * (E and M are summed across a wave: a decision whose two sides agree to ~1e-9 relative may fall
 * either way; every pixel is exact for the count its tile got.)                                  */
typedef struct mfx_adaptive {
    int32_t min_spp, max_spp, step_spp, reserved; /* 2 <= min <= max, step >= 1, reserved 0 */
    double rel_error;                             /* >= 0, finite */
    double abs_floor;                             /* >= 0, finite */
} mfx_adaptive; /* 32 bytes */

/* frame_xmajor_rgba: per-pixel mean over its tile's count, alpha 1 (layout of mfx_sample);
 * tile_spp: [tiles_y * tiles_x] the tiles' sample counts, row-major by tile row; rgba_ymajor: the
 * same mean through ACES -> sqrt -> RGBA8 (layout of mfx_render_rgba8). Each may be NULL.
 * The call clears and uses the context's accumulator and the two moment planes (allocated at the
 * first call: a context that never calls this pays nothing); the film (mfx_render_rgba8's state)
 * is left untouched. Afterwards the accumulator holds per-pixel sums over differing counts, so
 * mfx_accum_read_mean is meaningless until the next clear. mfx_ray_counts, mfx_stats,
 * mfx_last_trace_ms, mfx_trace_timing and mfx_ray_counts_total report the sum over the call's passes
 * (device time: the passes' traces and checks and the final mean). Always the wavefront pipeline.
 * MFX_E_INVALID: a bad struct or a NULL ctx. MFX_E_STATE: a context with part_count > 1,
 * MFX_F_ROW_PARTITION, a device list (ndevices > 0) or MFX_F_MEGAKERNEL (adaptive sampling over
 * several GPUs needs the tiles re-balanced between passes and is not provided).                */
int mfx_sample_adaptive(mfx_ctx* ctx, const mfx_adaptive* cfg, double* frame_xmajor_rgba, int32_t* tile_spp,
                        uint8_t* rgba_ymajor);

/* mfx_sample_adaptive_resume: continue the adaptive result the context holds, with this call's
 * thresholds and budget. Additive in ABI 6. The call clears nothing: it works on the accumulator,
 * S1 and S2, the tiles' counts n_T, B (the value next_sample had when that result's
 * mfx_sample_adaptive began) and R (the budget reserved so far: that call's max_spp, raised by every
 * later resume) as they are. E, M, m and the convergence test are mfx_sample_adaptive's, evaluated
 * at a tile's own count n_T.
 *  1. Entry check, no samples: every tile of the film is checked at its n_T under this call's
 *     rel_error and abs_floor; a tile is active iff it fails the test and n_T < max_spp. A tighter
 *     threshold re-activates tiles that had stopped; a looser one, or a max_spp at or below a
 *     tile's count, leaves the tile stopped.
 *  2. A pass: every active tile T gets cnt_T = min(step_spp, max_spp - n_T) samples, the global
 *     samples B + n_T .. B + n_T + cnt_T - 1, summed into the pixel's accumulator, S1 and S2 in
 *     sample order; then n_T += cnt_T and the tile is checked at its new n_T: it goes on iff it
 *     fails and n_T < max_spp. Tiles of one pass may have different n_T and different cnt_T.
 *  3. Passes repeat until no tile is active or max_passes passes have run (0: no limit).
 *     *active_out (may be NULL) is the number of tiles that would go on: always 0 when max_passes is 0.
 *  4. If max_spp > R, next_sample advances by max_spp - R and R becomes max_spp; otherwise the
 *     counter does not move. Later calls so draw samples no pixel has used.
 *  5. frame_xmajor_rgba, tile_spp, rgba_ymajor: as in mfx_sample_adaptive, each may be NULL; tile_spp
 *     is every tile's current count, active ones included, and a pixel is its samples
 *     B .. B + n_T - 1 summed in order and divided by n_T. The ray counters, mfx_stats, the trace
 *     times and the totals are as there: the sum over this call's passes (device time: the checks,
 *     the passes and the mean). A call that runs no pass reports 0 rays.
 *  6. Afterwards the context holds a valid adaptive result: mfx_denoise_var filters it
 *     (MFX_DN_SRC_ADAPTIVE) and another resume continues it.
 * Equivalence: one mfx_sample_adaptive call with (min, max, step, rel, floor) equals the call with
 * (min, min, step, rel, floor) followed by a resume with (max, step, max_passes 0, rel, floor): the
 * frame, the counts, the RGBA8, the moments, next_sample and the summed ray counters agree bit for
 * bit; so does the resume with max_passes 1 repeated until *active_out is 0 (the entry check of
 * each call repeats the verdicts of the check that ended the call before it).
 * Idempotence: a resume with the same thresholds and budget on a result that has none active traces
 * nothing and returns the same outputs: the check is deterministic for given moments and n.
 * MFX_E_INVALID: a NULL ctx or cfg, or a bad struct. MFX_E_STATE: whatever mfx_sample_adaptive
 * refuses (device list, part_count > 1, MFX_F_ROW_PARTITION, MFX_F_MEGAKERNEL); no valid adaptive
 * result (none yet, or a trace, mfx_accum_clear or mfx_accum_attach since); next_sample != B + R,
 * i.e. something else drew samples in between, such as a render call served by render-ahead.      */
typedef struct mfx_adaptive_resume {
    int32_t max_spp, step_spp, max_passes, reserved; /* max_spp >= 2, step_spp >= 1, max_passes >= 0 (0: no limit), reserved 0 */
    double rel_error, abs_floor;                     /* finite, >= 0 */
} mfx_adaptive_resume; /* 32 bytes */
int mfx_sample_adaptive_resume(mfx_ctx* ctx, const mfx_adaptive_resume* cfg, double* frame_xmajor_rgba,
                               int32_t* tile_spp, uint8_t* rgba_ymajor, int32_t* active_out);

/* ---- feature buffers and denoising (an extension: the reference shows the raw estimate) --------
 * Additive in ABI 6.
 *
 * mfx_aov: first-hit features of the film's own camera rays. For pixel (i, j) and global sample s the
 * ray is the path's: key pixel i*h + j, draws 0 and 1 of (seed, pixel, s) give u = (i + d0)/w,
 * v = (j + d1)/h, PinholeCamera.GetRay(u, v), then Bvh.Hit(ray, 1e-6, 99999999.), i.e. the first
 * vertex mfx_sample would shade. Per pixel, 8 doubles, each summed over s = sample_base ..
 * sample_base + spp - 1 in sample order from +0.0 (a miss adds nothing), then divided once by
 * (double)spp:
 *   [0..2] hit normal (as mfx_closest_hit returns it), [3] hit t, [4..6] albedo of the hit
 *   primitive's material, [7] 1.0 per hit (the hit fraction).
 * The planes stay on the device as the context's feature buffers (allocated at the first call: a
 * context that never calls this pays nothing) and are what mfx_denoise is guided by.
 * out_xmajor (may be NULL): out[(i*h + j)*8 + k].  ms (may be NULL): device time from HIP events.
 * The key takes s modulo 2^32, as in mfx_trace_accumulate: sample 2^32 + k gives sample k's ray.
 * Leaves the accumulator, the film, the moment planes, next_sample and every ray counter untouched.
 * MFX_E_INVALID: NULL ctx, spp < 1, sample_base < 0. MFX_E_STATE: part_count > 1,
 * MFX_F_ROW_PARTITION or a device list (as mfx_sample_adaptive). Flat and instanced scenes alike. */
int mfx_aov(mfx_ctx* ctx, int32_t spp, int64_t sample_base, double* out_xmajor, double* ms);

/* mfx_denoise: an edge-avoiding a-trous filter of a colour image, guided by the feature buffers.
 * C is the current colour (three channels; at first the source image), N, Z, A the feature buffers'
 * normal [0..2], depth [3] and albedo [4..6];
 *     d2(a,b) = ((a0-b0)*(a0-b0) + (a1-b1)*(a1-b1)) + (a2-b2)*(a2-b2),    k = [3/8, 1/4, 1/16].
 * For iteration i = 0 .. iterations-1 with step s = 2^i, for pixel p = (x, y):
 *   taps q = (x + dx*s, y + dy*s), dy = -2..2 in the outer loop, dx = -2..2 in the inner one; a tap
 *   outside the film is skipped. g = 1.0, then, in this order, for each term whose sigma is > 0,
 *   g = g * (1.0 / (1.0 + term)):
 *     normal:  term = d2(N_p, N_q) / (sn*sn)
 *     depth:   dz = Z_p - Z_q; den = (sz*sz) * (Z_p*Z_p + Z_q*Z_q); term = den > 0 ? (dz*dz)/den : 0
 *     albedo:  term = d2(A_p, A_q) / (sa*sa)
 *     colour:  term = d2(C_p, C_q) / ((sc*sc) * 0.25^i)          (0.25^i: an exact power of two)
 *   wt = (k[|dx|] * k[|dy|]) * g;  num_c = num_c + wt * C_q[c] and den = den + wt, both from +0.0 in
 *   tap order;  out_c = num_c / den (the centre tap has g = 1, so den >= 9/64).
 * The next iteration reads this output. Everything is FP64, one rounding per operation, no
 * contraction, and the weights are rational (+ - * / only, no exp), so a host statement of the rule
 * (mafrixraytracing_amd/denoise.py) gives the same bits. With every sigma 0 it is the plain B3-spline
 * a-trous transform's smoothing. There is no variance term here: soft shadow edges, which no feature
 * marks, blur as iterations grow (mfx_denoise_var below has one).                                 */
#define MFX_DN_SRC_HOST  0  /* color_in: a host frame in mfx_sample's layout (alpha ignored) */
#define MFX_DN_SRC_ACCUM 1  /* the context's accumulator / count (mfx_accum_read_mean's value); color_in NULL */
typedef struct mfx_denoise_cfg {
    int32_t iterations;        /* 1..8 */
    int32_t source;            /* MFX_DN_SRC_* */
    int32_t reserved[2];       /* 0 */
    double count;              /* SRC_ACCUM: > 0; SRC_HOST: ignored */
    double sigma_normal, sigma_depth, sigma_albedo, sigma_color; /* finite, >= 0; 0 switches the term off */
    /* A sigma > 0 must leave its term's divisor non-zero in FP64: sn*sn, sz*sz and sa*sa != 0 (a sigma
     * below about 1.5e-162 squares to 0), and (sc*sc) * 0.25^i != 0 for every i < iterations, 0.25^i by
     * repeated multiplication from 1.0. Otherwise the centre tap's term is 0/0: MFX_E_INVALID. */
} mfx_denoise_cfg; /* 56 bytes */
/* out_xmajor_rgba (mfx_sample's layout, alpha 1.0), rgba_ymajor (ACES -> sqrt -> RGBA8 of it,
 * mfx_render_rgba8's layout), ms (device time from HIP events): each may be NULL. Changes no context
 * state but its own two ping-pong colour buffers (allocated at the first call).
 * MFX_E_INVALID: a NULL ctx or cfg, a bad struct, SRC_HOST with NULL color_in, SRC_ACCUM with
 * count <= 0. MFX_E_STATE: as mfx_aov, and additionally when mfx_aov has not run on this context, or
 * not since the last mfx_set_camera (the features are another view's: run mfx_aov again).          */
int mfx_denoise(mfx_ctx* ctx, const mfx_denoise_cfg* cfg, const double* color_in,
                double* out_xmajor_rgba, uint8_t* rgba_ymajor, double* ms);

/* mfx_denoise_var: mfx_denoise's filter with a variance-guided luminance term, and the composition
 * of the adaptive sampler with it on the device. Additive in ABI 6.
 * C, N, Z, A, d2 and k are mfx_denoise's; V is the current variance of the pixel's mean luminance
 * (one plane; at first the source's), L(c) = (c0 + c1) + c2, k3 = [1/2, 1/4].
 * For iteration i = 0 .. iterations-1 with step s = 2^i, for pixel p = (x, y):
 *   1. variance prefilter, only when sigma_luma > 0: pn = pd = +0.0; for dy = -1..1 in the outer loop
 *      and dx = -1..1 in the inner one, q = (x + dx, y + dy) (always one pixel apart, whatever s is; a
 *      tap outside the film is skipped): kk = k3[|dx|] * k3[|dy|]; pn = pn + kk * V_q; pd = pd + kk.
 *      Vf = pn / pd;  lden = (sigma_luma*sigma_luma) * Vf + luma_floor.
 *   2. taps q = (x + dx*s, y + dy*s) exactly as in mfx_denoise (dy outer, dx inner, outside skipped):
 *      g = 1.0, then the normal, depth and albedo terms as there and in that order, then, if
 *      sigma_luma > 0:  dl = L(C_p) - L(C_q); term = (dl*dl) / lden; g = g * (1.0 / (1.0 + term)).
 *   3. wt = (k[|dx|] * k[|dy|]) * g;  num_c = num_c + wt * C_q[c], den = den + wt and
 *      vn = vn + (wt*wt) * V_q, all from +0.0 in tap order;  out_c = num_c / den,
 *      V'_p = vn / (den*den). The next iteration reads C' and V'.
 * FP64, one rounding per operation, no contraction, rational weights: the host statement
 * (mafrixraytracing_amd/denoise.py, reference_denoise_var) gives the same bits. With sigma_luma = 0
 * the colour is mfx_denoise's with sigma_color = 0 on the same frame and features, bit for bit; the
 * variance is still propagated. A pixel whose neighbourhood is noisy (large Vf) takes its
 * neighbours' luminance as it comes; one whose samples agree keeps an edge no feature marks.        */
#define MFX_DN_SRC_ADAPTIVE 2  /* the last mfx_sample_adaptive's result, as resumed since, on the device */
typedef struct mfx_denoise_var_cfg {
    int32_t iterations;   /* 1..8 */
    int32_t source;       /* MFX_DN_SRC_HOST, MFX_DN_SRC_ADAPTIVE or MFX_DN_SRC_TEMPORAL (below: mfx_temporal) */
    int32_t reserved[2];  /* 0 */
    double sigma_normal, sigma_depth, sigma_albedo, sigma_luma; /* finite, >= 0; 0 switches the term off */
    /* sigma_normal, sigma_depth, sigma_albedo > 0 must have a non-zero square in FP64, as for
     * mfx_denoise: MFX_E_INVALID otherwise. sigma_luma needs no such rule: lden >= luma_floor. */
    double luma_floor;    /* finite, > 0 */
} mfx_denoise_var_cfg;    /* 56 bytes */
/* MFX_DN_SRC_HOST: color_in is a frame in mfx_sample's layout (alpha ignored), variance_in[x*h + y]
 * w*h doubles (expected >= 0, not validated); both are required. MFX_DN_SRC_ADAPTIVE: both must be
 * NULL; with n = (double)tile_spp[tile of the pixel], C = accum / n (the frame mfx_sample_adaptive
 * or the last resume returned) and, from the moment planes, d = S2 - (S1*S1)/n, V = (d > 0 ? d : +0.0) / (n*(n - 1.0)):
 * the tile check's v_p.
 * out_xmajor_rgba, rgba_ymajor and ms are mfx_denoise's; var_out[x*h + y] is the last iteration's V'.
 * Each output may be NULL. The call changes no context state but buffers of its own (allocated at
 * its first call: two variance planes, and the colour buffers it shares with mfx_denoise): the
 * accumulator, the moment planes, the tiles' counts, the film, next_sample and every ray counter
 * are left untouched.
 * MFX_E_INVALID: a NULL ctx or cfg, a bad struct, pointers that do not fit the source.
 * MFX_E_STATE: as mfx_aov; when mfx_aov has not run on this context; MFX_DN_SRC_ADAPTIVE when the
 * accumulator does not hold an mfx_sample_adaptive result or its mfx_sample_adaptive_resume
 * continuation (none yet, or a trace, mfx_accum_clear, mfx_accum_attach or mfx_set_camera since);
 * feature buffers traced before the last mfx_set_camera (run mfx_aov again).                 */
int mfx_denoise_var(mfx_ctx* ctx, const mfx_denoise_var_cfg* cfg, const double* color_in,
                    const double* variance_in, double* out_xmajor_rgba, double* var_out,
                    uint8_t* rgba_ymajor, double* ms);

/* mfx_temporal: reproject the previous result into the current view and merge it with this frame's
 * samples (the temporal third of SVGF; the variance estimate and the a-trous filter are
 * mfx_denoise_var). Additive in ABI 6. Every material is traced as LambertianBrdf (Material.fs:52,
 * 68,121): a surface point's outgoing radiance does not depend on the view direction, so history
 * reprojected onto the same surface point estimates the same quantity.
 * Per pixel p = (x, y), q = x*h + y: this frame's colour C, variance of the mean luminance V and
 * sample count n (a double); the current feature planes N (normal), Z (depth), F (hit fraction) and
 * camera (o, tl, r, d); the history the context owns: colour HC, variance HV, effective count HN, its
 * view's features HNm, HZ, HF and camera (o', tl', r', d'). FP64, one rounding per operation, no
 * contraction; dot(a,b) = (a0*b0 + a1*b1) + a2*b2, cross by components a1*b2 - a2*b1, ..., d2 as above.
 *  1. No history (the first call, or restart != 0), or F != 1.0: reject.
 *  2. u = (x + 0.5)/w, v = (y + 0.5)/h; target = (tl + r*u) + d*v; dir = normalize(target - o) as
 *     mfx_aov normalizes its camera ray (l = sqrt(dot), each component / l); P = o + dir*Z.
 *  3. e = P - o', a = tl' - o', nn = cross(r', d'); den = dot(e, nn), num = dot(a, nn); reject unless
 *     num*den > 0. s = num/den, g = e*s - a; u' = dot(g, r')/dot(r', r'), v' = dot(g, d')/dot(d', d');
 *     reject unless 0 <= u' < 1 and 0 <= v' < 1. x' = min(w-1, (int)floor(u'*w)), y' likewise,
 *     q' = x'*h + y': the nearest history pixel. (u', v') is exactly the point's image for orthogonal
 *     r', d', which the constructor gives; with skewed `derived` axes it is the same arithmetic and only
 *     approximately the same point.
 *  4. At q': reject unless HF == 1.0; ze = sqrt(dot(e, e)), dz = ze - HZ; reject unless
 *     dz*dz <= (tol_depth*tol_depth)*(ze*ze); reject unless d2(N_p, HNm_q') <= tol_normal2.
 *  5. Accept: nh = HN_q' < max_history ? HN_q' : max_history, nt = n + nh, wc = n/nt, wh = nh/nt;
 *     C'_c = wc*C_c + wh*HC_c, V' = (wc*wc)*V + (wh*wh)*HV, N' = nt. On a reject C' = C, V' = V, N' = n.
 *  6. Afterwards the history is (C', V', N') with the current features and camera (two buffers that
 *     swap by pointer: the gather reads q' while q is written).
 * The host statement of the rule is mafrixraytracing_amd/temporal.py, reference_temporal: the same bits. */
#define MFX_DN_SRC_TEMPORAL 3  /* mfx_denoise_var: the temporal history's C' and V', where they lie on the device */
typedef struct mfx_temporal_cfg {
    int32_t source;        /* MFX_DN_SRC_HOST or MFX_DN_SRC_ADAPTIVE */
    int32_t restart;       /* != 0: ignore and replace the history */
    int32_t reserved[2];   /* 0 */
    double tol_depth;      /* finite, >= 0: relative depth tolerance (0 accepts only dz == 0) */
    double tol_normal2;    /* finite, >= 0: bound on d2 of the normals */
    double max_history;    /* finite, > 0: cap on the history's weight, in samples */
} mfx_temporal_cfg;        /* 40 bytes */
/* MFX_DN_SRC_HOST: color_in is a frame in mfx_sample's layout (alpha ignored), variance_in[x*h + y]
 * and count_in[x*h + y] w*h doubles each; all three are required; count_in must be finite and is
 * expected > 0, variance_in >= 0 (neither validated). MFX_DN_SRC_ADAPTIVE: all three must be NULL; C and
 * V are exactly mfx_denoise_var's reading of the adaptive result and n = (double)tile_spp[tile].
 * out_xmajor_rgba, rgba_ymajor and ms are mfx_denoise_var's, of C'; var_out[x*h + y] = V',
 * count_out[x*h + y] = N', *accepted = the pixels that took history. Each output may be NULL.
 * mfx_denoise_var with source MFX_DN_SRC_TEMPORAL then filters C' and V' (host pointers NULL);
 * it returns MFX_E_STATE without a history, or with one merged under another camera epoch than the
 * feature buffers'. The history is kept across mfx_set_camera: that is its purpose.
 * The call changes nothing but its own buffers (two history buffers of 10 planes, one count plane,
 * allocated at the first call; mfx_denoise_var's first colour and variance buffers as staging).
 * MFX_E_INVALID: a NULL ctx or cfg, a bad struct, pointers that do not fit the source. MFX_E_STATE:
 * whatever mfx_aov refuses: a device list, partitions; no mfx_aov yet, or none since the last mfx_set_camera;
 * MFX_DN_SRC_ADAPTIVE without a valid adaptive result.                                             */
int mfx_temporal(mfx_ctx* ctx, const mfx_temporal_cfg* cfg, const double* color_in, const double* variance_in,
                 const double* count_in, double* out_xmajor_rgba, double* var_out, double* count_out,
                 uint8_t* rgba_ymajor, int64_t* accepted, double* ms);

/* == Film.GetFrame(integrator, spp) + Scene.PostProcessAndToScreenBuffer
 * (Film.fs:18-34, Scene.fs:315-333): adds spp samples per pixel to the film, then writes the
 * progressive mean through ACES -> sqrt -> int(255.99 c) as RGBA8, y-major:
 * rgba[(y*w + x)*4 + {0,1,2,3}]. `Scene.Render(delta, buffer)` is this call with spp = 1.
 * rgba may be NULL (accumulate only).
 * Render-ahead (mfx_options.render_ahead = K > 1, part_count 1): one-sample calls are
 * served from batches of K samples. A call whose global sample is not held traces the next K
 * samples in one batched pass that runs the film add and post of all K calls ahead, in call
 * order; each call of the batch then only copies its RGBA8 frame, and while a batch is served the
 * next one is traced in the background (two buffers of K x 4 B + 48 B per pixel). Every frame's
 * bytes and the film equal the one-sample path's (a sample's image depends only on the seed and
 * its global index); after mfx_reset, an spp != 1 call or mfx_sample the next one-sample call
 * traces a batch again from the film as it then is. mfx_stats: the first call
 * served from a batch reports the K samples' rays and device time, the others 0 rays in 0 s. The
 * two buffers take at most MFX_RENDER_AHEAD_MAX_BYTES (environment; default 2 GiB) and a quarter of
 * the free HBM: K is cut to fit two buffers while at least 8 samples fit in each (1080p: 2 x 64 in 1.26 GB),
 * else one buffer of as many samples as fit (no background batch); when not even two samples fit,
 * the context frees the buffers and renders one sample per call from then on. A background batch
 * is traced once a batch starts being served, so an application that stops early has traced at
 * most one batch ahead. The accumulator (mfx_accum_read_mean) does not hold the samples of calls
 * served from batches. On a device list every device serves its tile rows from its own batches
 * (the same K on each: the tightest device's budget, shared by a list's contexts on one GPU).
 * mfx_film_mean after calls served mid-batch traces each served sample again once, film only.   */
int mfx_render_rgba8(mfx_ctx* ctx, int32_t spp, uint8_t* rgba_ymajor);

/* The same call under SURVEY.md §8(b)'s name for it (Film.GetFrame + PostProcess). */
int mfx_accumulate_render_rgba8(mfx_ctx* ctx, int32_t spp, uint8_t* rgba_ymajor);

/* == Film.Reset (Film.fs:26-30): zero the film accumulator and its frame count. */
int mfx_reset(mfx_ctx* ctx);

/* Film mean (target texture, Film.fs:23) as x-major RGBA doubles. */
int mfx_film_mean(mfx_ctx* ctx, double* frame_xmajor_rgba);

/* ---- lower-level entry points (multi-GPU composition, benchmarking) -------------------- */

/* Adds, for global samples [sample_base, sample_base + spp) of this context's partition,
 * the per-pixel radiance sums into the context's device accumulator (FP64, 3 planes of w*h,
 * plane-major, x-major pixels); on a multi-device context each device into its own.
 * Does not synchronise; mfx_sync() does.
 * Global sample indices are 64-bit, and the path key takes them modulo 2^32:
 * global sample 2^32 + k is sample k again, so a range that crosses 2^32 continues with
 * samples 0, 1, ...                                                                           */
int mfx_trace_accumulate(mfx_ctx* ctx, int32_t spp, int64_t sample_base);
/* Multi-device context: sum every device's accumulator into the primary's (RCCL reduce, root
 * devices[0]), ordered after each device's trace: after a clear and a trace, an exact merge of
 * the devices' tile rows. No-op on a single-device context, and on an accumulator already merged
 * since the last trace, clear or attach. mfx_sample calls it itself.                             */
int mfx_accum_reduce(mfx_ctx* ctx);
int mfx_accum_clear(mfx_ctx* ctx);
/* Device pointer + byte size of the (primary device's) FP64 accumulator (for an RCCL reduce
 * across ranks).                                                                             */
int mfx_accum_device_ptr(mfx_ctx* ctx, void** dptr, int64_t* nbytes);
/* Use caller-owned device memory (>= the size above, on this context's device) as the
 * accumulator — e.g. a buffer an RCCL reduce then works on in place; NULL restores the
 * context's own buffer. The caller keeps it alive until detached or mfx_destroy.            */
int mfx_accum_attach(mfx_ctx* ctx, void* dptr, int64_t nbytes);
/* Copy accumulator / count to host as x-major RGBA doubles (alpha = 1): the division by the
 * sample count itself, as `color / float n` (Integrators.fs:171). count must be > 0. On a device
 * list it reads the merged accumulator: a trace not merged since (mfx_trace_accumulate, or the
 * trace of an mfx_render_rgba8 call without render-ahead) is merged first (mfx_accum_reduce).   */
int mfx_accum_read_mean(mfx_ctx* ctx, double count, double* frame_xmajor_rgba);
int mfx_sync(mfx_ctx* ctx);
/* The HIP stream (hipStream_t) the context launches on, for event timing by the caller.   */
int mfx_stream(mfx_ctx* ctx, void** stream);

/* Device time (ms) of the last mfx_trace_accumulate, from HIP events recorded on the
 * context's stream around its kernels (waits for them to finish).                           */
int mfx_last_trace_ms(mfx_ctx* ctx, double* ms);

/* Per-stage device time of the last mfx_trace_accumulate (wavefront pipeline), summed over its
 * iterations from HIP events around each kernel: out[0] = whole call, out[2] = the closest-hit
 * kernels (path start + closest hit: k_camera and k_extend), out[4] = k_shadow (shading + shadow
 * ray + path finish); out[1] = the part of out[2] spent in k_camera (each generation's camera
 * rays traced as packets, flat scenes) and out[3] = its launches (0 when k_extend traced them);
 * the per-generation k_resolve launches make up the rest of out[0]; out[5] = iterations
 * (max_depth + 1 per generation), out[6] = launches of each stage (= out[5]), out[7] =
 * generations. Megakernel: out[0] = out[2] = its single launch.                               */
int mfx_trace_timing(mfx_ctx* ctx, double out[8]);

/* Ray counters of the last mfx_trace_accumulate / mfx_sample call:
 * out[0] = primary, out[1] = extension (closest-hit queries actually traced, excluding the
 * reference's discarded depth -1 query), out[2] = shadow, out[3] = paths; with
 * MFX_F_COUNT_STATS: out[4..6] = internal-node visits, cluster (reference leaf) visits and
 * primitive tests of the closest-hit queries, out[7..9] the same for the shadow queries, and
 * out[10] / out[11] = the camera-ray packets' own fetches (k_camera: wave-uniform 128-B node
 * steps and leaf slots, once per wave; the per-ray visits of packet lanes are in out[4..6]).    */
int mfx_ray_counts(mfx_ctx* ctx, double out[16]);

/* The same counters summed over every mfx_trace_accumulate (and mfx_sample / mfx_render_rgba8
 * without render-ahead) since the context was created or last reset: each trace adds its counters
 * to device-side totals in stream order, so back-to-back traces need no host read in between (the
 * benchmark's timed steps). Waits for the context's work; reset != 0 zeroes the totals after the read. */
int mfx_ray_counts_total(mfx_ctx* ctx, double out[16], int32_t reset);

/* SURVEY.md §8(b)'s stats call, for the Mrays/s metric (§8(d)): rays = primary + extension +
 * shadow rays traced by the last mfx_sample / mfx_render_rgba8 / mfx_trace_accumulate call (the
 * sum of mfx_ray_counts out[0..2]), seconds = its device time (mfx_last_trace_ms / 1000; waits
 * for the call's kernels). Either pointer may be NULL.                                        */
int mfx_stats(mfx_ctx* ctx, double* rays, double* seconds);

/* ---- query entry points (parity tests of the BVH/intersection layer) ----------------- */

/* Closest hit, == Bvh.Hit(ray, tmin, tmax) (BvhNode.fs:62-83) for n rays given as
 * rays[k*6 + 0..2] = origin, [3..5] = unit direction. Outputs t (0 when no hit), prim index
 * (-1 when no hit; index into the mfx_prim array), and the hit normal.                      */
int mfx_closest_hit(mfx_ctx* ctx, int64_t n, const double* rays, double tmin, double tmax,
                    double* t_out, int32_t* prim_out, double* normal_out);
/* Shadow query, == Bvh.Hit(...).hit with per-ray tmax: occluded[k] = 1/0.                  */
int mfx_any_hit(mfx_ctx* ctx, int64_t n, const double* rays, double tmin, const double* tmax,
                int32_t* occluded_out);

/* Reference heap-BVH leaf grouping used for the exact leaf semantics (BvhNode.fs:24-61):
 * indices[nprims] after Subdivide; leaf_first/leaf_count per reference leaf in heap order.  */
int mfx_ref_leaves(mfx_ctx* ctx, int32_t* indices_out, int32_t* leaf_first_out,
                   int32_t* leaf_count_out, int32_t* nleaves_out);

/* Host-only (no device needed): the same leaf grouping computed straight from a scene
 * description, plus the traversal BVH's shape: info[0] = clusters, info[1] = internal BVH4
 * nodes, info[2] = LDS stack entries per lane, info[3] = traversal slots. Any output pointer
 * may be NULL.                                                                                */
int mfx_build_leaves(const mfx_scene_desc* scene, int32_t* indices_out, int32_t* leaf_first_out,
                     int32_t* leaf_count_out, int32_t* nleaves_out, int32_t info_out[4]);

/* How mfx_create built the scene (Scene ctor, Scene.fs:298-313; Bvh.Build, BvhNode.fs:24-61):
 * out[0] = ms for the reference leaf grouping (host), out[1] = ms for the traversal BVH2
 * (GPU incl. transfers, or host; with the GPU image layout: the whole traversal image), out[2] = ms
 * for the whole scene preparation, out[3] = 1 if the BVH2 was built on the GPU, 2 if its BVH4
 * collapse and image layout ran there too (flat scenes), out[4] = BVH4 nodes, out[5] = traversal slots, out[6] = BVH2
 * internal nodes, out[7] = BVH2 build levels. digest (may be NULL) = FNV-1a of the device
 * images (nodes, slots, slot_ref, ref_blob, shade): equal digests mean identical traversal.    */
int mfx_build_info(mfx_ctx* ctx, double out[8], uint64_t* digest);

/* Device FP64 self-test: computes a/b, sqrt(a) on the GPU for n pairs (bit-exactness check
 * of the device math the numerics contract relies on).                                      */
int mfx_fp64_selftest(int32_t device, int64_t n, const double* a, const double* b,
                      double* div_out, double* sqrt_out);

/* Device self-test of the exact shortcuts the traversal puts in front of AABB.hit
 * (IHitable.fs:18-54): rec = n records of 24 doubles (lo[3], hi[3], origin[3], direction[3],
 * tMin, tMax, a triangle's v0[3], e1[3], e2[3] whose vertex box lies inside [lo, hi], one pad);
 * out = 3 int32 per record: the FP64 test's answer (0/1), the FP32 screen's (1 hit, 0 miss, -1
 * left to the FP64 test) and the vertex-box proof's (1 proved to pass, 0 not proved; plus 2 if the
 * proof's plain and folded forms, which must agree, do not). Wherever a shortcut decides it must
 * agree with the FP64 answer.                                                                  */
int mfx_aabb_selftest(int32_t device, int64_t n, const double* rec, int32_t* out);

/* How a context's work is laid over devices (ABI 6, additive): out[0] = devices G, out[1] = RCCL
 * communicators the context created (G for a list of distinct devices, else 0), out[2] = how
 * mfx_accum_reduce merges (0 one device, 1 RCCL reduce, 2 device-ordered adds: a repeated device),
 * out[3] / out[4] = the primary's tile-row band (band_index, band_count: the serpentine band
 * band_index), out[5 + g] = device g's HIP ordinal. cap = entries of out (>= 5 + G).          */
int mfx_device_info(mfx_ctx* ctx, int32_t* out, int32_t cap);

/* The launch shape the context's creation chose for its wavefront kernels and the megakernel (ABI 6,
 * additive): which template instances run and on what grids, the MFX_* tuning variables applied
 * and clamped. cap = entries of out (>= MFX_LAUNCH_INFO_N). The primary device's values:
 * out[0] = traversal-stack bound (entries per lane), out[1] / out[2] = of which in LDS in k_extend /
 * k_shadow, out[3] / out[4] = 1 if k_extend / k_shadow run their spill instances (deeper entries in
 * a global column), out[5] / out[6] = top BVH nodes in LDS (k_extend / k_shadow), out[7] / out[8] =
 * slots in LDS (> 0: the small-scene instances), out[9] = instance records in LDS (two-level
 * scenes; the others are read from global memory), out[10] = k_shadow's build (3 or 4 waves per
 * SIMD), out[11] = the megakernel's (1 or 4), out[12] = 1 if a HIT state word carries the lit mask,
 * out[13] = 1 if a lit vertex's direct term is recorded as one double (a gray light; 0 with several
 * lights), out[14] = 1 if camera rays run as packets, out[15] / out[16] / out[17] = blocks of k_extend /
 * k_shadow / k_camera
 * (0: no packets), out[18] = the spill buffer's entries per lane, out[19] = the lanes it holds,
 * out[20] = slots per chunk fetch, out[21] = 1 if k_shadow takes half chunks on small frames,
 * out[22] = the first iteration that moves paths to a ray queue (-1 never, -2 automatic),
 * out[23] = path slots of the pool at most (saturated at 2^31 - 1).
 * The camera cuts (camera packets that start from a per-tile cut of the BVH, cached per camera; off
 * with MFX_CAMERA_CUTS=0, on two-level scenes and without camera packets): out[24] = 1 if they are in
 * use, out[25] = entries per tile (MFX_CAMERA_CUT_CAP), out[26] = bytes of the table, and of the last
 * table built on the primary device (0 before the first; the call waits for a build in flight):
 * out[27] = 1000 x its mean cut length, out[28] = its longest cut, out[29] = its tiles whose cut is the
 * root alone; out[30] = tables built so far, out[31] = the fewest samples of a trace that builds one
 * (MFX_CAMERA_CUT_MIN_SAMPLES; a table that is already the camera's serves every trace).        */
#define MFX_LAUNCH_INFO_N 32
int mfx_launch_info(mfx_ctx* ctx, int32_t* out, int32_t cap);
/* The primary device's camera-cut table for the current camera: rows [tile ty * tiles_x + tx][out[25]
 * of mfx_launch_info] of 32-byte entries {int32 code, float lb, float lo[3], float hi[3]} (code >= 0 an
 * internal node, < 0 a leaf, INT32_MIN after a row's last entry). host == 0: the device's table, built
 * now if it is not this camera's; host != 0: the same routine run on the host over the host image (the
 * two are equal byte for byte). *nbytes = the table's size; out may be NULL to ask for it alone.
 * MFX_E_STATE when the context does not use cuts, MFX_E_INVALID: cap_bytes < *nbytes.           */
int mfx_camera_cut_table(mfx_ctx* ctx, void* out, int64_t cap_bytes, int64_t* nbytes, int32_t host);
/* The primary device's last camera-cut build (waits for one in flight; all 0 without cuts or before the
 * first): out[0] = tables built so far, out[1] = the last build's device time in ms (HIP events),
 * out[2] = the sum of its cut lengths, out[3] = the longest, out[4] = tiles whose cut is the root
 * alone, out[5] = tiles with an empty cut, out[6] = film tiles, out[7] = entries per tile,
 * out[8 + n] = tiles whose cut has n entries (n = 0 .. 16); the per-tile slot cull, over the leaf
 * entries the cuts took in: out[25] = their slots, out[26] = slots their entries no longer hold,
 * out[27] = entries dropped whole, out[28] = entries narrowed (all 0 for a table built without the
 * cull: one whose camera has served fewer than MFX_CAMERA_CUT_CULL_MIN_SAMPLES samples, 128 by
 * default), out[29] = 1 if the current table was built with the cull; the rest 0.              */
int mfx_camera_cut_info(mfx_ctx* ctx, double out[32]);

/* ---- misc -------------------------------------------------------------------------------- */
const char* mfx_last_error(void);
int mfx_abi_version(void);
int mfx_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MAFRIX_RT_H */
