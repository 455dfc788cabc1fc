// vx_obj.h -- the OBJ (+ MTL) reader of vx_obj.cpp, as vx_api.cpp calls it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/voxhip.h"

namespace vx {

// what attribute shading reads besides positions and faces (vx_obj.cpp)
struct ObjAttributes {
    std::vector<float> nrm, uv;          // 9 / 6 floats per triangle, corner k of triangle t at 3t + k; empty when the file has no vn / vt line
    std::vector<std::string> tex_names;  // one per texture slot: the map_Kd files, in material order
    std::vector<int32_t> mat_slot;       // per material: its slot or -1
};

// returns 0 ok, 1 file missing/unreadable, 2 parse error (msg filled); attr (optional) is filled on success only
int load_obj(const char* path, std::vector<float>& verts, std::vector<int32_t>& tris, std::vector<int32_t>& tri_mat, std::vector<vx_material>& mats,
             std::string& msg, ObjAttributes* attr);

}  // namespace vx
