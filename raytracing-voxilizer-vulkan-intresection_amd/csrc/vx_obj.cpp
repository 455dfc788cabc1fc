// vx_obj.cpp -- Wavefront OBJ (+ MTL) reader for what the voxelizer consumes: positions, faces, per-face material ids.
//
// Stands where the reference calls tinyobj::ObjReader::ParseFromFile (VoxelBuilder.hpp:59-69, octTree.hpp:304-314):
// the hot path reads attrib.vertices (xyz float32), per shape in file order mesh.indices[].vertex_index in triples, and --
// in the material plumbing the reference keeps commented out (VoxelBuilder.hpp:375-395) -- mesh.material_ids[face] and the
// material_t records (ior, dissolve, shininess, illum, ambient, diffuse, specular, transmittance, emission).  Shapes are
// flattened in order, which is the order both reference drivers walk them in.
// Corner attributes (attribute shading of frames, include/voxhip.h): `vt` / `vn` lines and the vt / vn index of every face corner, stored per
// corner of the fanned triangles (corner k of triangle t at 3t + k) as common/obj_loader.cpp:76-86 keeps them, uv = (u, 1 - v); and map_Kd of
// the MTL, one texture slot per material that has one, in material order (obj_loader.cpp:49-52).  A vt / vn index that is 0 or out of range
// only leaves that attribute absent: positions, triangles, materials and every error are those of the same file without attributes.
// tinyobjloader itself is third-party and absent from the reference tree (unpinned version); this reader accepts the same
// `v` / `f` / `usemtl` / `mtllib` grammar (v, v/vt, v//vn, v/vt/vn, negative = relative indices, polygons fan-triangulated,
// positive indices may refer to vertices defined later in the file) and parses numbers locale-independently
// (std::from_chars, bounded to the line) -> float.  OBJ-text parity with tinyobj's own number parser / polygon
// triangulation is not pinned by anything in the reference; fixtures use `f i j k` triangles and %.9g floats only.
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/voxhip.h"
#include "vx_obj.h"

namespace vx {

static inline const char* skip_ws(const char* p, const char* eol) { while (p < eol && (*p == ' ' || *p == '\t')) ++p; return p; }

// one decimal number in [q, eol); never reads past the line, never consults the C locale.  A numeral beyond double's range reads as
// +-Inf, one below it as +-0 (include/voxhip.h, "OBJ numerals"): from_chars leaves `out` untouched on result_out_of_range, so the
// value comes from the numeral's own text -- the decimal exponent of its first non-zero digit, which is far from 0 on either side.
static bool parse_real(const char*& q, const char* eol, double& out)
{
    const char* s = q;
    if (s < eol && *s == '+') ++s;  // from_chars rejects an explicit plus sign
    double d = 0.0;
    const std::from_chars_result r = std::from_chars(s, eol, d);
    if (r.ec != std::errc() && r.ec != std::errc::result_out_of_range) return false;
    if (r.ptr == s) return false;
    if (r.ec == std::errc::result_out_of_range) {
        const char* p = s;
        const bool neg = *p == '-';
        if (neg) ++p;
        long long lead = 0;  // decimal exponent of the first non-zero digit, before the explicit exponent
        bool point = false, found = false;
        for (; p < r.ptr && *p != 'e' && *p != 'E'; ++p) {
            if (*p == '.') { point = true; continue; }
            if (!found) {
                if (*p != '0') { found = true; lead = point ? lead - 1 : 0; }
                else if (point) --lead;
            } else if (!point) ++lead;
        }
        long long ex = 0;
        if (p < r.ptr) {  // e[+-]digits, saturated: the sign of the sum is all that is read
            ++p;
            const bool eneg = p < r.ptr && *p == '-';
            if (p < r.ptr && (*p == '-' || *p == '+')) ++p;
            for (; p < r.ptr; ++p) ex = ex < 1000000000LL ? ex * 10 + (*p - '0') : ex;
            if (eneg) ex = -ex;
        }
        d = lead + ex > 0 ? HUGE_VAL : 0.0;
        if (neg) d = -d;
    }
    out = d;
    q = r.ptr;
    return true;
}

// double -> float, rounded to nearest as the conversion does it inside float's range; beyond it, where the conversion is undefined,
// +-Inf at or above FLT_MAX + half an ulp (2^128 - 2^103) and +-FLT_MAX below
static float to_float(double d)
{
    constexpr double fmax = (double)std::numeric_limits<float>::max();
    constexpr double lim = 340282356779733661637539395458142568448.0;
    if (d > fmax) return d >= lim ? std::numeric_limits<float>::infinity() : std::numeric_limits<float>::max();
    if (d < -fmax) return d <= -lim ? -std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::max();
    return (float)d;  // NaN converts to NaN
}

static std::string token(const char*& q, const char* eol)
{
    q = skip_ws(q, eol);
    const char* b = q;
    while (q < eol && *q != ' ' && *q != '\t' && *q != '\r') ++q;
    return std::string(b, q);
}

static bool read_file(const char* path, std::string& data)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) data.append(buf, n);
    std::fclose(f);
    return true;
}

// tinyobj's material_t defaults (InitMaterial): everything zero except dissolve, shininess and ior = 1
static vx_material default_mtl()
{
    vx_material m;
    std::memset(&m, 0, sizeof(m));
    m.shininess = 1.0f;
    m.ior = 1.0f;
    m.dissolve = 1.0f;
    m.illum = 0;
    m.texture_id = -1;
    return m;
}

// .mtl: newmtl / Ka Kd Ks Kt|Tf Ke Ns Ni d|Tr illum, and map_Kd.  Texture maps are not on the voxel path (textureID stays -1 as in
// the reference's copy, VoxelBuilder.hpp:383-394): the file of map_Kd (its last token, options skipped, relative to the MTL's directory)
// goes to tex_path, one entry per material, empty without a map_Kd.
static void load_mtl(const std::string& path, std::vector<vx_material>& mats, std::unordered_map<std::string, int>& by_name,
                     std::vector<std::string>& tex_path)
{
    std::string data;
    if (!read_file(path.c_str(), data)) return;  // tinyobj: a missing .mtl is a warning, faces keep material id -1
    const char* p = data.c_str();
    const char* end = p + data.size();
    int cur = -1;
    std::string mdir(path);
    {
        const size_t slash = mdir.find_last_of("/\\");
        mdir = slash == std::string::npos ? std::string() : mdir.substr(0, slash + 1);
    }
    while (p < end) {
        const char* eol = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        if (!eol) eol = end;
        const char* q = p;
        const std::string key = token(q, eol);
        auto vec3 = [&](float* dst) {
            for (int k = 0; k < 3; ++k) {
                q = skip_ws(q, eol);
                double d;
                if (!parse_real(q, eol, d)) break;
                dst[k] = to_float(d);
            }
        };
        auto real1 = [&](float& dst) {
            q = skip_ws(q, eol);
            double d;
            if (parse_real(q, eol, d)) dst = to_float(d);
        };
        if (key == "newmtl") {
            const std::string name = token(q, eol);
            mats.push_back(default_mtl());
            tex_path.emplace_back();
            cur = (int)mats.size() - 1;
            by_name.emplace(name, cur);  // first definition of a name wins, as in tinyobj's map insert
        } else if (cur >= 0) {
            vx_material& m = mats[(size_t)cur];
            if (key == "Ka") vec3(m.ambient);
            else if (key == "Kd") vec3(m.diffuse);
            else if (key == "Ks") vec3(m.specular);
            else if (key == "Kt" || key == "Tf") vec3(m.transmittance);
            else if (key == "Ke") vec3(m.emission);
            else if (key == "Ns") real1(m.shininess);
            else if (key == "Ni") real1(m.ior);
            else if (key == "d") real1(m.dissolve);
            else if (key == "Tr") { float tr = 0.0f; real1(tr); m.dissolve = 1.0f - tr; }
            else if (key == "illum") { float v = 0.0f; real1(v); m.illum = (v > -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : 0; }
            else if (key == "map_Kd") {
                std::string last;
                for (std::string t = token(q, eol); !t.empty(); t = token(q, eol)) last = t;
                if (!last.empty()) tex_path[(size_t)cur] = (last[0] == '/' ? std::string() : mdir) + last;
            }
        }
        p = eol + 1;
    }
}

// one integer of a corner's vt / vn field at q; false (nothing consumed past digits) when there is none
static bool corner_index(const char*& q, const char* eol, long long& v)
{
    const char* s = q;
    if (s < eol && *s == '+') ++s;
    const std::from_chars_result r = std::from_chars(s, eol, v);
    if (r.ec != std::errc() || r.ptr == s) return false;
    q = r.ptr;
    return true;
}

// a vt / vn reference: 1-based, negative = relative to the lines read so far; -1 = absent (0, before the first line); checked against the
// final count at the end (a positive index may point further down the file, as for positions)
static int64_t attr_ref(long long vi, int64_t nsofar)
{
    if (vi > 0) return vi - 1;
    if (vi < 0 && nsofar + vi >= 0) return nsofar + vi;
    return -1;
}

// returns 0 ok, 1 file missing/unreadable, 2 parse error (msg filled); attr (optional) filled on success
int load_obj(const char* path, std::vector<float>& verts, std::vector<int32_t>& tris, std::vector<int32_t>& tri_mat, std::vector<vx_material>& mats,
             std::string& msg, ObjAttributes* attr)
{
    std::string data;
    if (!read_file(path, data)) { msg = "Path does not exist!"; return 1; }
    verts.clear();
    tris.clear();
    tri_mat.clear();
    mats.clear();
    std::unordered_map<std::string, int> mat_by_name;
    std::string dir(path);
    {
        const size_t slash = dir.find_last_of("/\\");
        dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
    }
    std::vector<int64_t> poly, poly_vt, poly_vn;
    std::vector<int64_t> corner_vt, corner_vn;  // per corner of every triangle: the vt / vn line it names (-1 none)
    std::vector<float> vts, vns;                // vt (u, v) and vn (x, y, z) lines
    std::vector<std::string> tex_path;          // per material: its map_Kd file or empty
    std::vector<size_t> tri_line;  // line of every triangle, for the range check after the last vertex is known
    int cur_mat = -1;
    const char* p = data.c_str();
    const char* end = p + data.size();
    size_t line_no = 0;
    while (p < end) {
        ++line_no;
        const char* eol = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        if (!eol) eol = end;
        const char* q = skip_ws(p, eol);
        if (q + 1 < eol && q[0] == 'v' && (q[1] == ' ' || q[1] == '\t')) {
            q += 2;
            float xyz[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < 3; ++k) {
                q = skip_ws(q, eol);
                double d;
                if (!parse_real(q, eol, d)) break;
                xyz[k] = to_float(d);
            }
            verts.push_back(xyz[0]); verts.push_back(xyz[1]); verts.push_back(xyz[2]);
        } else if (q + 2 < eol && q[0] == 'v' && (q[1] == 't' || q[1] == 'n') && (q[2] == ' ' || q[2] == '\t')) {
            const int nc = q[1] == 't' ? 2 : 3;  // vt u [v [w]]: a missing v is 0 / vn x y z
            q += 3;
            float c[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < nc; ++k) {
                q = skip_ws(q, eol);
                double d;
                if (!parse_real(q, eol, d)) break;
                c[k] = to_float(d);
            }
            std::vector<float>& dst = nc == 2 ? vts : vns;
            dst.insert(dst.end(), c, c + nc);
        } else if (q + 1 < eol && q[0] == 'f' && (q[1] == ' ' || q[1] == '\t')) {
            q += 2;
            poly.clear();
            poly_vt.clear();
            poly_vn.clear();
            const int64_t nv = (int64_t)(verts.size() / 3);  // negative indices are relative to the vertices read so far
            for (;;) {
                q = skip_ws(q, eol);
                if (q >= eol || *q == '\r' || *q == '#') break;
                long long vi = 0;
                const char* s = q;
                if (s < eol && *s == '+') ++s;
                const std::from_chars_result r = std::from_chars(s, eol, vi);
                if (r.ec != std::errc() || r.ptr == s) { msg = "malformed face at line " + std::to_string(line_no); return 2; }
                q = r.ptr;
                long long ti = 0, ni = 0;  // v/vt, v//vn, v/vt/vn: anything else in the corner is skipped as before
                if (q < eol && *q == '/') {
                    ++q;
                    if (!corner_index(q, eol, ti)) ti = 0;
                    if (q < eol && *q == '/') {
                        ++q;
                        if (!corner_index(q, eol, ni)) ni = 0;
                    }
                }
                poly_vt.push_back(attr_ref(ti, (int64_t)(vts.size() / 2)));
                poly_vn.push_back(attr_ref(ni, (int64_t)(vns.size() / 3)));
                while (q < eol && *q != ' ' && *q != '\t' && *q != '\r') ++q;
                int64_t idx;
                if (vi > 0) idx = vi - 1;  // may point at a vertex further down the file: checked at the end
                else if (vi < 0) {
                    idx = nv + vi;
                    if (idx < 0) { msg = "face index out of range at line " + std::to_string(line_no); return 2; }
                } else { msg = "face index 0 at line " + std::to_string(line_no); return 2; }
                if (idx > 0x7FFFFFFE) { msg = "face index out of range at line " + std::to_string(line_no); return 2; }
                poly.push_back(idx);
            }
            for (size_t k = 2; k < poly.size(); ++k) {
                tris.push_back((int32_t)poly[0]);
                tris.push_back((int32_t)poly[k - 1]);
                tris.push_back((int32_t)poly[k]);
                for (size_t c : {(size_t)0, k - 1, k}) { corner_vt.push_back(poly_vt[c]); corner_vn.push_back(poly_vn[c]); }
                tri_mat.push_back(cur_mat);
                tri_line.push_back(line_no);
            }
        } else if (eol - q > 7 && std::strncmp(q, "usemtl", 6) == 0 && (q[6] == ' ' || q[6] == '\t')) {
            q += 7;
            const std::string name = token(q, eol);
            const auto it = mat_by_name.find(name);
            cur_mat = it == mat_by_name.end() ? -1 : it->second;  // unknown name: tinyobj warns and leaves the faces without material
        } else if (eol - q > 7 && std::strncmp(q, "mtllib", 6) == 0 && (q[6] == ' ' || q[6] == '\t')) {
            q += 7;
            for (;;) {
                const std::string name = token(q, eol);
                if (name.empty()) break;
                load_mtl(dir + name, mats, mat_by_name, tex_path);
            }
        }
        p = eol + 1;
    }
    const int64_t nv = (int64_t)(verts.size() / 3);
    for (size_t t = 0; t < tris.size(); ++t)
        if (tris[t] >= nv) { msg = "face index out of range at line " + std::to_string(tri_line[t / 3]); return 2; }
    if (attr) {
        const size_t nc = tris.size();
        const int64_t nvt = (int64_t)(vts.size() / 2), nvn = (int64_t)(vns.size() / 3);
        attr->uv.clear();
        attr->nrm.clear();
        if (nvt) {  // a corner without a (valid) vt: (0, 0)
            attr->uv.assign(nc * 2, 0.0f);
            for (size_t c = 0; c < nc; ++c)
                if (corner_vt[c] >= 0 && corner_vt[c] < nvt) {
                    attr->uv[2 * c] = vts[2 * corner_vt[c]];
                    attr->uv[2 * c + 1] = 1.0f - vts[2 * corner_vt[c] + 1];  // obj_loader.cpp:84
                }
        }
        if (nvn) {  // attrib.normals non-empty: corner normals; a corner without a (valid) vn: (0, 0, 0)
            attr->nrm.assign(nc * 3, 0.0f);
            for (size_t c = 0; c < nc; ++c)
                if (corner_vn[c] >= 0 && corner_vn[c] < nvn)
                    for (int k = 0; k < 3; ++k) attr->nrm[3 * c + k] = vns[3 * corner_vn[c] + k];
        }
        attr->tex_names.clear();
        attr->mat_slot.assign(mats.size(), -1);
        for (size_t i = 0; i < mats.size(); ++i)
            if (!tex_path[i].empty()) {
                attr->mat_slot[i] = (int32_t)attr->tex_names.size();
                attr->tex_names.push_back(tex_path[i]);
            }
    }
    return 0;
}

}  // namespace vx
