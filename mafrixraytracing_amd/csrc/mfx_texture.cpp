// mfx_texture.cpp — albedo textures on the host (include/mafrix_rt.h, mfx_create_textured): what is refused,
// the texture descriptors, the UV table of the world primitives, and the two host-only calls that expose
// the code creation runs (mfx_uv_table, mfx_texel_index). No device is touched here.
#include "mfx_ctx.h"

using namespace mfxh;

static_assert(sizeof(mfx_texture) == 16 && sizeof(mfx_prim_uv) == 56, "the ABI's texture structs");
static_assert(MFX_MAX_TEXTURES == MFX_TEX_COUNT_MAX && MFX_MAX_TEXTURE_DIM == MFX_TEX_DIM_MAX, "the ABI's bounds are the kernels'");

// From the sizes alone (no texel and no rgba pointer is looked at): the count, every width and height, the
// total; desc[t].base = texels before texture t.
bool mfx_texture_descs(const mfx_texture* textures, int ntextures, std::vector<MfxTexDesc>& desc, int64_t& ntexels,
                       std::string& err) {
    desc.clear();
    ntexels = 0;
    if (ntextures < 0 || ntextures > MFX_MAX_TEXTURES) {
        err = "ntextures " + std::to_string(ntextures) + " is outside 0 .. " + std::to_string(MFX_MAX_TEXTURES);
        return false;
    }
    if (ntextures > 0 && !textures) {
        err = "null texture array with ntextures > 0";
        return false;
    }
    for (int t = 0; t < ntextures; ++t) {
        const int32_t w = textures[t].width, h = textures[t].height;
        if (w < 1 || w > MFX_MAX_TEXTURE_DIM || h < 1 || h > MFX_MAX_TEXTURE_DIM) {
            err = "texture " + std::to_string(t) + " is " + std::to_string(w) + " x " + std::to_string(h) +
                  ": width and height must be 1 .. " + std::to_string(MFX_MAX_TEXTURE_DIM);
            return false;
        }
    }
    for (int t = 0; t < ntextures; ++t) {
        desc.push_back(MfxTexDesc{(int32_t)ntexels, textures[t].width, textures[t].height, 0});
        ntexels += (int64_t)textures[t].width * textures[t].height;
        if (ntexels > MFX_TEXELS_MAX) {
            err = "texture " + std::to_string(t) + " brings the texels to more than 2^31 - 2 in all";
            return false;
        }
    }
    return true;
}

// one template primitive's map: the first offender, or true
static bool check_prim_uv(const mfx_prim& p, const mfx_prim_uv& m, int64_t i, int ntextures, std::string& err) {
    const std::string who = "primitive " + std::to_string(i);
    if (m.texture < -1 || m.texture >= ntextures) {
        err = who + " has texture " + std::to_string(m.texture) + ", outside -1 .. " + std::to_string(ntextures - 1);
        return false;
    }
    if (m.texture < 0) return true;
    if (p.kind == MFX_PRIM_SPHERE) {
        err = who + " is a textured sphere (spheres have no UV map)";
        return false;
    }
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 2; ++a)
            if (!std::isfinite(m.uv[k][a])) {
                err = who + " uv of corner " + std::to_string(k) + " is not finite";
                return false;
            }
    return true;
}

bool mfx_prepare_textures(const mfx_scene_desc* scene, const mfx_instance* instances, int ninstances,
                          const mfx_texture* textures, int ntextures, const mfx_prim_uv* prim_uv, MfxTexHost& out,
                          std::string& err) {
    out = MfxTexHost{};
    if (!mfx_texture_descs(textures, ntextures, out.desc, out.ntexels, err)) return false;
    for (int t = 0; t < ntextures; ++t)
        if (!textures[t].rgba) {
            err = "texture " + std::to_string(t) + " has a null rgba";
            return false;
        }
    if (ntextures > 0 && !prim_uv) {
        err = "null prim_uv with ntextures > 0";
        return false;
    }
    if (!prim_uv) return true;  // no texture and no map: an untextured scene
    if (!scene || !scene->prims || scene->nprims < 1) return true;  // (mfx_build_scene names what is wrong with it)
    bool any = false;
    for (int64_t i = 0; i < scene->nprims; ++i) {
        if (!check_prim_uv(scene->prims[i], prim_uv[i], i, ntextures, err)) return false;
        any = any || prim_uv[i].texture >= 0;
    }
    if (!any) return true;
    // the world primitives, and the template each came from: the expansion in entry order (mfx_instance)
    std::vector<mfx_prim> world;
    std::vector<int64_t> from;
    const mfx_prim* wp = scene->prims;
    int64_t nw = scene->nprims;
    if (instances) {
        if (!mfx_expand(scene->prims, scene->nprims, instances, ninstances, world, err)) return false;
        for (int k = 0; k < ninstances; ++k)
            for (int64_t i = 0; i < instances[k].count; ++i) from.push_back(instances[k].first + i);
        wp = world.data();
        nw = (int64_t)world.size();
    }
    out.ptex.assign((size_t)nw, -1);
    out.uvrec.assign((size_t)nw * MFX_UV_RECORD_DOUBLES, 0.0);
    for (int64_t w = 0; w < nw; ++w) {
        const mfx_prim_uv& m = prim_uv[instances ? from[(size_t)w] : w];
        if (m.texture < 0) continue;
        out.ptex[(size_t)w] = m.texture;
        mfx_tx_record(wp[w].p[0], wp[w].p[1], wp[w].p[2], m.uv, &out.uvrec[(size_t)w * MFX_UV_RECORD_DOUBLES]);
        out.on = true;
    }
    if (!out.on) {  // (textured templates that no instance uses)
        out.ptex.clear();
        out.uvrec.clear();
    }
    return true;
}

extern "C" {
int mfx_uv_table(const mfx_prim* prims, int64_t nprims, const mfx_prim_uv* prim_uv, double* out) {
    if (!prims || !prim_uv || !out || nprims < 0) return fail(MFX_E_INVALID, "mfx_uv_table: null argument");
    for (int64_t i = 0; i < nprims; ++i) {
        double* r = out + i * MFX_UV_RECORD_DOUBLES;
        if (prim_uv[i].texture < 0 || prims[i].kind == MFX_PRIM_SPHERE) std::fill(r, r + MFX_UV_RECORD_DOUBLES, 0.0);
        else mfx_tx_record(prims[i].p[0], prims[i].p[1], prims[i].p[2], prim_uv[i].uv, r);
    }
    return MFX_OK;
}

int mfx_texel_index(const mfx_texture* textures, int32_t ntextures, int32_t texture, int64_t n, const double* uv,
                    uint32_t* id_out) {
    std::vector<MfxTexDesc> desc;
    int64_t ntexels = 0;
    std::string err;
    if (!mfx_texture_descs(textures, ntextures, desc, ntexels, err)) return fail(MFX_E_INVALID, "mfx_texel_index: " + err);
    if (texture < 0 || texture >= ntextures)
        return fail(MFX_E_INVALID, "mfx_texel_index: texture " + std::to_string(texture) + " is outside 0 .. " +
                                       std::to_string(ntextures - 1));
    if (n < 0 || (n > 0 && (!uv || !id_out))) return fail(MFX_E_INVALID, "mfx_texel_index: null argument");
    for (int64_t k = 0; k < n; ++k) id_out[k] = mfx_tx_texel(desc[(size_t)texture], uv[2 * k], uv[2 * k + 1]);
    return MFX_OK;
}
}
