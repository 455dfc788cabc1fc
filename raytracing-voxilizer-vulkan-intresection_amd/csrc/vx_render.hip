// vx_render.hip -- the per-pixel work of a frame between and after the traversals (vx_render_frame_device): the camera block, the merge of the
// voxel and triangle hits with the shadow ray of each pixel, and the shading of raytrace.rchit:49-143 / raytrace2.rchit:53-137 with the miss
// colour of raytrace.rmiss:37 and the gamma of post.frag:36.  The arithmetic is cpp/voxilizer.cpp render()'s, operation for operation, so
// that the device frame is that function's picture:
//   * the primary direction in render()'s host association: tg = norm(((pi0*dx + pi4*dy) + pi8) + pi12, ...) with norm DIVIDING by the
//     length, dir = (vi0*tg.x + vi4*tg.y) + vi8*tg.z -- not load_ray's (a+b)+(c+d) and multiply-by-inverse;
//   * hit point org + dir*t, the triangle's interpolated position (p0*b0 + p1*b1) + p2*b2 with b0 = (1 - b1) - b2, the light vector, its
//     length sqrtf(dot) and L = l * (1/dist).
// Shadow-ray origin, direction and tMax are bit-equal to the host's only if every float operation rounds as the host's does.  Under build.py's
// flags (-ffp-contract=off, -fno-fast-math, plus the file's fp contract pragma) nothing is fused, and hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt makes `/` and sqrtf correctly rounded (v_div_scale / v_div_fmas / v_div_fixup, and the
// v_sqrt_f32 sequence with its two correction steps, in the ISA; no v_rcp_f32 or bare v_sqrt_f32 result is used).  powf (the specular
// term and the gamma) is the one operation whose last bit may differ from the host's libm: at most 1 LSB in the 8-bit result.
#include "vx_internal.h"

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr unsigned kRenderBlock = 256;

// The camera arrives by value as a kernel argument (copied at enqueue time): no host copy that must outlive the call, no synchronise.
__global__ __launch_bounds__(64) void k_render_camera(Camera cam, Camera* out)
{
    if (threadIdx.x == 0) *out = cam;
}

// render()'s primary direction of pixel r (voxilizer.cpp: u, v, dx, dy, tg = norm(...), dirs[i])
__device__ __forceinline__ void host_dir(const Camera& cam, uint64_t r, float& d0, float& d1, float& d2)
{
    const uint32_t px = (uint32_t)(r % cam.width), py = (uint32_t)(r / cam.width);
    const float u = ((float)px + 0.5f) / (float)cam.width, v = ((float)py + 0.5f) / (float)cam.height;
    const float dx = u * 2.f - 1.f, dy = v * 2.f - 1.f;
    const float* p = cam.projInv;
    const float t0 = ((p[0] * dx + p[4] * dy) + p[8]) + p[12];
    const float t1 = ((p[1] * dx + p[5] * dy) + p[9]) + p[13];
    const float t2 = ((p[2] * dx + p[6] * dy) + p[10]) + p[14];
    const float l = sqrtf((t0 * t0 + t1 * t1) + t2 * t2);
    const float g0 = t0 / l, g1 = t1 / l, g2 = t2 / l;
    const float* m = cam.viewInv;
    d0 = (m[0] * g0 + m[4] * g1) + m[8] * g2;
    d1 = (m[1] * g0 + m[5] * g1) + m[9] * g2;
    d2 = (m[2] * g0 + m[6] * g1) + m[10] * g2;
}

__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// the closer hit; the voxel on equal t (render(): tri = mt > 0 && !(t > 0 && t <= mt))
__device__ __forceinline__ bool is_tri(float vt, const float* mt, uint64_t r) { return mt && mt[r] > 0.f && !(vt > 0.f && vt <= mt[r]); }

// the normal the shading uses: the voxel's cube normal, or the triangle's geometric normal turned toward the ray
__device__ __forceinline__ void shade_normal(bool tri, const RenderParams& P, uint64_t r, float d0, float d1, float d2, float& n0, float& n1, float& n2)
{
    const float* nb = tri ? P.mnrm : P.vnrm;
    n0 = nb[3 * r]; n1 = nb[3 * r + 1]; n2 = nb[3 * r + 2];
    if (tri && dot3(n0, n1, n2, d0, d1, d2) > 0.0f) { n0 = n0 * -1.0f; n1 = n1 * -1.0f; n2 = n2 * -1.0f; }
}

// A pixel's triangle hit, resolved once per site: the mesh it belongs to (0, or the instance's BLAS), that mesh's vertices and index triples,
// the instance, and the barycentrics in the pinned form b0 = 1 - b1 - b2.  What a site does not read costs nothing.
struct TriHit {
    uint32_t mesh, inst;
    const float* verts;
    const int32_t* idx;
    float b0, b1, b2;
};
template <bool kInst>
__device__ __forceinline__ TriHit tri_hit(const RenderParams& P, uint64_t r)
{
    TriHit h{0, 0, P.verts, P.idx, 0.0f, P.mbary[2 * r], P.mbary[2 * r + 1]};
    if (kInst) {
        h.inst = P.minst[r];
        h.mesh = P.iblas[h.inst];
        const InstMesh& im = P.imesh[h.mesh];
        h.verts = im.verts;
        h.idx = im.idx;
    }
    h.b0 = 1.0f - h.b1 - h.b2;
    return h;
}

// Attribute shading (include/voxhip.h): the unit normal N of a triangle hit -- the corner normals interpolated ((n0*b0 + n1*b1) +
// n2*b2, or the face normal cross(p1 - p0, p2 - p0) without them), moved to world space by W^T n for an instance ((w0j*n0 + w1j*n1) + w2j*n2),
// then n / sqrtf(dot(n, n)), NOT turned toward the ray (raytrace.rchit:73-74).  A zero-length or non-finite N: the default normal.
template <bool kInst>
__device__ __forceinline__ void attr_normal(const RenderParams& P, const AttrParams& A, uint64_t r, float d0, float d1, float d2, float& n0, float& n1,
                                            float& n2)
{
    const uint32_t k = P.mprim[r];
    const TriHit h = tri_hit<kInst>(P, r);
    const AttrMesh* am = A.mesh + h.mesh;
    const float b0 = h.b0, b1 = h.b1, b2 = h.b2;
    float x, y, z;
    if (am->nrm) {
        const float* c = am->nrm + 9ull * k;
        x = (c[0] * b0 + c[3] * b1) + c[6] * b2;
        y = (c[1] * b0 + c[4] * b1) + c[7] * b2;
        z = (c[2] * b0 + c[5] * b1) + c[8] * b2;
    } else {
        const int32_t* ti = h.idx + 3 * (uint64_t)k;
        const float* p0 = h.verts + 3 * (uint64_t)ti[0];
        const float* p1 = h.verts + 3 * (uint64_t)ti[1];
        const float* p2 = h.verts + 3 * (uint64_t)ti[2];
        const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
        const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
        x = e1y * e2z - e1z * e2y;
        y = e1z * e2x - e1x * e2z;
        z = e1x * e2y - e1y * e2x;
    }
    if (kInst) {
        const float* w = A.w2o + 12ull * h.inst;
        const float ox = x, oy = y, oz = z;
        x = (w[0] * ox + w[4] * oy) + w[8] * oz;
        y = (w[1] * ox + w[5] * oy) + w[9] * oz;
        z = (w[2] * ox + w[6] * oy) + w[10] * oz;
    }
    const float len = sqrtf((x * x + y * y) + z * z);
    const float N0 = x / len, N1 = y / len, N2 = z / len;
    if (isfinite(N0) && isfinite(N1) && isfinite(N2) && !(N0 == 0.0f && N1 == 0.0f && N2 == 0.0f)) {
        n0 = N0; n1 = N1; n2 = N2;
    } else {
        shade_normal(true, P, r, d0, d1, d2, n0, n1, n2);
    }
}

template <bool kInst, bool kAttr>
__device__ __forceinline__ void render_shadow_rays(const RenderParams& P, const AttrParams& A)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.n) return;
    const Camera& cam = *P.cam;
    const float vt = (!kInst || P.vt) ? P.vt[r] : -1.0f;
    const bool tri = is_tri(vt, P.mt, r);
    float d0, d1, d2;
    host_dir(cam, r, d0, d1, d2);
    const float ts = tri ? P.mt[r] : (vt > 0.f ? vt : 0.f);
    const float w0 = cam.viewInv[12] + d0 * ts, w1 = cam.viewInv[13] + d1 * ts, w2 = cam.viewInv[14] + d2 * ts;
    float l0, l1, l2;
    if (P.light_type == 1) {  // directional (rchit:86-91): L = normalize(lightPosition), lightDistance 100000
        l0 = P.light[0]; l1 = P.light[1]; l2 = P.light[2];
    } else if (tri) {          // rchit:67-68,78-83: from the position the barycentrics interpolate
        const uint32_t k = P.mprim[r];
        const TriHit h = tri_hit<kInst>(P, r);  // an instance's mesh; its object-to-world rows below (rchit:70, gl_ObjectToWorldEXT)
        const int32_t* ti = h.idx + 3 * (uint64_t)k;
        const float b0 = h.b0, b1 = h.b1, b2 = h.b2;
        const float* p0 = h.verts + 3 * (uint64_t)ti[0];
        const float* p1 = h.verts + 3 * (uint64_t)ti[1];
        const float* p2 = h.verts + 3 * (uint64_t)ti[2];
        float h0 = p0[0] * b0 + p1[0] * b1 + p2[0] * b2;
        float h1 = p0[1] * b0 + p1[1] * b1 + p2[1] * b2;
        float h2 = p0[2] * b0 + p1[2] * b1 + p2[2] * b2;
        if (kInst) {  // M * p in the pinned association ((m0*x + m1*y) + m2*z) + m3
            const float* m = P.ixf + 12ull * h.inst;
            const float x = h0, y = h1, z = h2;
            h0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            h1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            h2 = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        }
        l0 = P.light[0] - h0;
        l1 = P.light[1] - h1;
        l2 = P.light[2] - h2;
    } else {
        l0 = P.light[0] - w0; l1 = P.light[1] - w1; l2 = P.light[2] - w2;
    }
    const float len = sqrtf(dot3(l0, l1, l2, l0, l1, l2));
    const float inv = 1.0f / len;
    const float L0 = l0 * inv, L1 = l1 * inv, L2 = l2 * inv;
    const float dist = P.light_type == 1 ? 100000.0f : len;
    float2* rp = reinterpret_cast<float2*>(P.srays + 6 * r);
    rp[0] = make_float2(w0, w1);
    rp[1] = make_float2(w2, L0);
    rp[2] = make_float2(L1, L2);
    P.sdist[r] = dist;
    float an0 = 0.f, an1 = 0.f, an2 = 0.f;
    if (kAttr && tri) {  // computed once per pixel: the compaction below and the shading read the same N
        attr_normal<kInst>(P, A, r, d0, d1, d2, an0, an1, an2);
        A.nbuf[3 * r] = an0; A.nbuf[3 * r + 1] = an1; A.nbuf[3 * r + 2] = an2;
    }
    // compaction by empty intervals: only a hit facing the light can read its shadow flag
    bool active = tri || vt > 0.f;
    if (active) {
        float n0, n1, n2;
        if (kAttr && tri) { n0 = an0; n1 = an1; n2 = an2; }
        else shade_normal(tri, P, r, d0, d1, d2, n0, n1, n2);
        active = dot3(n0, n1, n2, L0, L1, L2) > 0.0f;
    }
    P.stmax[r] = active ? dist : 0.0f;  // tmax 0 < tmin 0.001: no hit can be accepted
}

__global__ __launch_bounds__(kRenderBlock) void k_render_shadow_rays(RenderParams P) { render_shadow_rays<false, false>(P, AttrParams{}); }
__global__ __launch_bounds__(kRenderBlock) void k_render_shadow_rays_tlas(RenderParams P) { render_shadow_rays<true, false>(P, AttrParams{}); }
__global__ __launch_bounds__(kRenderBlock) void k_render_shadow_rays_attr(RenderParams P, AttrParams A) { render_shadow_rays<false, true>(P, A); }
__global__ __launch_bounds__(kRenderBlock) void k_render_shadow_rays_attr_tlas(RenderParams P, AttrParams A) { render_shadow_rays<true, true>(P, A); }

// MaterialObj{} (obj_loader.h:32-43): the fields the shading reads
__device__ __forceinline__ void load_material(const vx_material* tab, int64_t i, uint64_t n, float amb[3], float dif[3], float spc[3], float& shin, int& illum)
{
    if (i >= 0 && (uint64_t)i < n) {
        const vx_material& m = tab[i];
        for (int k = 0; k < 3; ++k) { amb[k] = m.ambient[k]; dif[k] = m.diffuse[k]; spc[k] = m.specular[k]; }
        shin = m.shininess;
        illum = m.illum;
    } else {
        amb[0] = amb[1] = amb[2] = 0.1f;
        dif[0] = dif[1] = 1.0f; dif[2] = 0.0f;
        spc[0] = spc[1] = spc[2] = 1.0f;
        shin = 0.0f;
        illum = 0;
    }
}

__device__ __forceinline__ uint32_t gamma8(float c)
{
    const float g = powf(fminf(fmaxf(c, 0.f), 1.f), 1.0f / 2.2f);  // post.frag:36
    return (uint32_t)lroundf(g * 255.0f);
}

// one axis of the bilinear lookup with repeat addressing: x = u*w - 0.5, the two texels floor(x) mod w and the next, the weight f = x - floor(x);
// x non-finite or |x| >= 2^62: texel 0 with weight 0
__device__ __forceinline__ void tex_axis(float u, uint32_t w, uint32_t& i0, uint32_t& i1, float& f)
{
    const float x = u * (float)w - 0.5f;
    if (!(fabsf(x) < 0x1p62f)) { i0 = i1 = 0; f = 0.0f; return; }
    const float fl = floorf(x);
    f = x - fl;
    int64_t m;
    if (fabsf(fl) < 0x1p31f) m = (int64_t)((int32_t)fl % (int32_t)w);  // the common case in 32-bit arithmetic: the same residue
    else m = (int64_t)fl % (int64_t)w;
    if (m < 0) m += w;
    i0 = (uint32_t)m;
    i1 = i0 + 1 == w ? 0u : i0 + 1;
}

// the texture of the triangle hit's material multiplies the diffuse term (raytrace.rchit:99-104): bilinear at the base level from RGBA8
// texels decoded through the sRGB table (lut, in LDS), float weights, alpha ignored
template <bool kInst>
__device__ __forceinline__ void attr_texture(const RenderParams& P, const AttrParams& A, const float* lut, uint64_t r, int64_t mi, float diff[3])
{
    // (the mesh lookup as it was before tri_hit, and tri_hit only behind the early returns: A.mesh + h.mesh from one call up here changes
    // k_render_shade_attr's instructions)
    const AttrMesh* am = kInst ? A.mesh + P.iblas[P.minst[r]] : A.mesh;
    if (mi < 0 || (uint64_t)mi >= am->nslot) return;
    const int32_t slot = am->slot[mi];
    if (slot < 0 || (uint32_t)slot >= am->ntex) return;
    const uint32_t k = P.mprim[r];
    const TriHit h = tri_hit<kInst>(P, r);
    const float b0 = h.b0, b1 = h.b1, b2 = h.b2;
    float u = 0.0f, v = 0.0f;
    if (am->uv) {
        const float* c = am->uv + 6ull * k;
        u = (c[0] * b0 + c[2] * b1) + c[4] * b2;
        v = (c[1] * b0 + c[3] * b1) + c[5] * b2;
    } else {
        u = (0.0f * b0 + 0.0f * b1) + 0.0f * b2;
        v = u;
    }
    const TexRec t = am->tex[slot];
    uint32_t x0, x1, y0, y1;
    float fx, fy;
    tex_axis(u, t.w, x0, x1, fx);
    tex_axis(v, t.h, y0, y1, fy);
    const uint32_t* base = A.texels + t.offset;
    const uint32_t t00 = base[(uint64_t)y0 * t.w + x0], t10 = base[(uint64_t)y0 * t.w + x1];
    const uint32_t t01 = base[(uint64_t)y1 * t.w + x0], t11 = base[(uint64_t)y1 * t.w + x1];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t sh = 8 * c;
        const float a = lut[(t00 >> sh) & 255u] * gx + lut[(t10 >> sh) & 255u] * fx;
        const float b = lut[(t01 >> sh) & 255u] * gx + lut[(t11 >> sh) & 255u] * fx;
        diff[c] = diff[c] * (a * gy + b * fy);
    }
}

template <bool kInst, bool kAttr>
__device__ __forceinline__ void render_shade(const RenderParams& P, const AttrParams& A, const float* lut)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.n) return;
    const float vt = (!kInst || P.vt) ? P.vt[r] : -1.0f;
    const bool tri = is_tri(vt, P.mt, r);
    const bool hit = tri || vt > 0.f;
    float c[3] = {0.8f, 0.8f, 0.8f};  // rmiss:37 with the white clear colour of main.cpp:184
    if (hit) {
        float d0, d1, d2, n0, n1, n2;
        host_dir(*P.cam, r, d0, d1, d2);
        if (kAttr && tri) { n0 = A.nbuf[3 * r]; n1 = A.nbuf[3 * r + 1]; n2 = A.nbuf[3 * r + 2]; }
        else shade_normal(tri, P, r, d0, d1, d2, n0, n1, n2);
        const float2* rp = reinterpret_cast<const float2*>(P.srays + 6 * r);
        const float2 a = rp[1], b = rp[2];
        const float L0 = a.y, L1 = b.x, L2 = b.y;
        const float dist = P.sdist[r];
        int64_t mi = -1;
        uint64_t nmat = 0;
        const vx_material* tab = nullptr;
        if (tri && kInst) {  // rchit:52,92-93: objDesc[gl_InstanceCustomIndexEXT] -> the instance's mesh's material of the triangle
            const InstMesh& im = P.imesh[tri_hit<kInst>(P, r).mesh];
            if (im.mids) mi = im.mids[P.mprim[r]];
            tab = im.mat; nmat = im.nmat;
        } else if (tri) {  // rchit:92-93: the triangle's OBJ material
            if (P.mids) mi = P.mids[P.mprim[r]];
            tab = P.mmat; nmat = P.nmmat;
        } else if (P.vids) {  // matIndices.i[gl_PrimitiveID] -> materials.m[matIdx]
            const uint32_t prim = P.vprim[r];
            if (prim < P.nvids) mi = P.vids[prim];
            tab = P.vmat; nmat = P.nvmat;
        }
        float amb[3], dif[3], spc[3], shin;
        int illum;
        load_material(tab, mi, nmat, amb, dif, spc, shin, illum);
        const float li = P.light_type == 1 ? P.intensity : P.intensity / (dist * dist);  // rchit:83 / :85
        const float dnl0 = dot3(n0, n1, n2, L0, L1, L2);
        const float dnl = fmaxf(dnl0, 0.0f);                                            // computeDiffuse, wavefront.glsl:25
        float diff[3] = {dif[0] * dnl, dif[1] * dnl, dif[2] * dnl};
        if (illum >= 1) { diff[0] += amb[0]; diff[1] += amb[1]; diff[2] += amb[2]; }
        if (kAttr && tri) attr_texture<kInst>(P, A, lut, r, mi, diff);  // after the ambient term, as rchit:99-104
        const bool lit = dnl0 > 0.0f;
        const bool shadowed = lit && ((P.sv && P.sv[r]) || (P.sm && P.sm[r]));
        float att = tri ? 1.0f : 0.3f;  // unlit: 1 for a triangle (rchit:106-140), 0.3 for a voxel (raytrace2.rchit:99-133)
        float spec[3] = {0.f, 0.f, 0.f};
        if (lit) {
            att = shadowed ? 0.3f : 1.0f;
            if (!shadowed && illum >= 2) {  // computeSpecular, wavefront.glsl:32-48
                const float kPi = 3.14159265f, kSh = fmaxf(shin, 4.0f);
                const float kE = (2.0f + kSh) / (2.0f * kPi);
                const float e0 = d0 * -1.0f, e1 = d1 * -1.0f, e2 = d2 * -1.0f;
                const float el = sqrtf(dot3(e0, e1, e2, e0, e1, e2));
                const float V0 = e0 / el, V1 = e1 / el, V2 = e2 / el;
                const float I0 = L0 * -1.0f, I1 = L1 * -1.0f, I2 = L2 * -1.0f;
                const float s = 2.0f * dot3(n0, n1, n2, I0, I1, I2);
                const float R0 = I0 - n0 * s, R1 = I1 - n1 * s, R2 = I2 - n2 * s;
                const float sp = kE * powf(fmaxf(dot3(V0, V1, V2, R0, R1, R2), 0.0f), kSh);
                spec[0] = spc[0] * sp; spec[1] = spc[1] * sp; spec[2] = spc[2] * sp;
            }
        }
        for (int k = 0; k < 3; ++k) c[k] = li * att * (diff[k] + spec[k]);
        if (P.shadowed_out) P.shadowed_out[r] = shadowed ? 1 : 0;
    }
    if (!hit && P.shadowed_out) P.shadowed_out[r] = 0;
    P.rgba[r] = gamma8(c[0]) | (gamma8(c[1]) << 8) | (gamma8(c[2]) << 16) | 0xFF000000u;  // one 32-bit store per pixel
    if (P.kind_out) P.kind_out[r] = tri ? 2 : (hit ? 1 : 0);
}

__global__ __launch_bounds__(kRenderBlock) void k_render_shade(RenderParams P) { render_shade<false, false>(P, AttrParams{}, nullptr); }
__global__ __launch_bounds__(kRenderBlock) void k_render_shade_tlas(RenderParams P) { render_shade<true, false>(P, AttrParams{}, nullptr); }

// the sRGB table goes to LDS first: one entry per thread of the 256-thread block, before any thread of the block leaves
static_assert(kRenderBlock == 256, "one sRGB table entry per thread");
template <bool kInst>
__device__ __forceinline__ void render_shade_attr(const RenderParams& P, const AttrParams& A)
{
    __shared__ float lut[256];
    lut[threadIdx.x] = A.srgb[threadIdx.x];
    __syncthreads();
    render_shade<kInst, true>(P, A, lut);
}
__global__ __launch_bounds__(kRenderBlock) void k_render_shade_attr(RenderParams P, AttrParams A) { render_shade_attr<false>(P, A); }
__global__ __launch_bounds__(kRenderBlock) void k_render_shade_attr_tlas(RenderParams P, AttrParams A) { render_shade_attr<true>(P, A); }

}  // namespace

void launch_render_camera(const Camera& cam, Camera* dev, hipStream_t s)
{
    VX_KL(k_render_camera, dim3(1), dim3(64), 0, s, cam, dev);
}

namespace {
dim3 render_grid(uint64_t n) { return dim3((unsigned)((n + kRenderBlock - 1) / kRenderBlock)); }
}  // namespace

// A: attribute shading's tables, or null for the default shading; inst: an instanced scene (P.minst / ixf / iblas / imesh set)
void launch_render_shadow_rays(const RenderParams& P, const AttrParams* A, bool inst, hipStream_t s)
{
    if (!P.n) return;
    const dim3 g = render_grid(P.n), b(kRenderBlock);
    if (A && inst) VX_KL(k_render_shadow_rays_attr_tlas, g, b, 0, s, P, *A);
    else if (A) VX_KL(k_render_shadow_rays_attr, g, b, 0, s, P, *A);
    else if (inst) VX_KL(k_render_shadow_rays_tlas, g, b, 0, s, P);
    else VX_KL(k_render_shadow_rays, g, b, 0, s, P);
}

void launch_render_shade(const RenderParams& P, const AttrParams* A, bool inst, hipStream_t s)
{
    if (!P.n) return;
    const dim3 g = render_grid(P.n), b(kRenderBlock);
    if (A && inst) VX_KL(k_render_shade_attr_tlas, g, b, 0, s, P, *A);
    else if (A) VX_KL(k_render_shade_attr, g, b, 0, s, P, *A);
    else if (inst) VX_KL(k_render_shade_tlas, g, b, 0, s, P);
    else VX_KL(k_render_shade, g, b, 0, s, P);
}

}  // namespace vx
