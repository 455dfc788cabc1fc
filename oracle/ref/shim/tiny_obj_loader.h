// Stand-in for tinyobjloader, written for this project: the types and the ObjReader calls the reference's voxelizer
// files use.  It reads `v x y z` (extra components ignored) and `f a b c ...` (the vertex index before any `/`,
// 1-based or negative = relative to the vertices read so far, as tinyobj's fixIndex), fan-triangulating polygons;
// every other statement (vn, vt, o, g, usemtl, mtllib, s, comments) is skipped and all faces land in one shape.
// Numbers go strtod -> float: exact for the %.9g float32 text the project's fixtures write.  tinyobj's own number
// parser and its n-gon triangulation are NOT reproduced (fixtures use triangles only).
#pragma once

#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

namespace tinyobj {

using real_t = float;

struct index_t {
    int vertex_index = -1;
    int normal_index = -1;
    int texcoord_index = -1;
};

struct attrib_t {
    std::vector<real_t> vertices;
    std::vector<real_t> vertex_weights;
    std::vector<real_t> normals;
    std::vector<real_t> texcoords;
    std::vector<real_t> colors;
};

struct mesh_t {
    std::vector<index_t> indices;
    std::vector<unsigned char> num_face_vertices;
    std::vector<int> material_ids;
    std::vector<unsigned int> smoothing_group_ids;
};

struct shape_t {
    std::string name;
    mesh_t mesh;
};

struct material_t {
    std::string name;
    real_t ambient[3] = {0, 0, 0};
    real_t diffuse[3] = {0, 0, 0};
    real_t specular[3] = {0, 0, 0};
    real_t transmittance[3] = {0, 0, 0};
    real_t emission[3] = {0, 0, 0};
    real_t shininess = 1;
    real_t ior = 1;
    real_t dissolve = 1;
    int illum = 0;
    std::string diffuse_texname;
};

struct ObjReaderConfig {
    bool triangulate = true;
    std::string mtl_search_path;
};

class ObjReader {
public:
    bool ParseFromFile(const std::string& filename, const ObjReaderConfig& = ObjReaderConfig())
    {
        std::ifstream in(filename);
        if (!in) {
            error_ = "Cannot open file [" + filename + "]\n";
            valid_ = false;
            return false;
        }
        shape_t shape;
        std::string line;
        std::vector<int> face;
        while (std::getline(in, line)) {
            const char* p = line.c_str();
            while (*p == ' ' || *p == '\t') ++p;
            if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
                p += 2;
                char* end = nullptr;
                for (int k = 0; k < 3; ++k) {
                    const double d = std::strtod(p, &end);
                    attrib_.vertices.push_back(static_cast<real_t>(d));
                    p = end;
                }
            } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
                p += 2;
                face.clear();
                const int nv = static_cast<int>(attrib_.vertices.size() / 3);
                while (true) {
                    while (*p == ' ' || *p == '\t') ++p;
                    if (*p == '\0' || *p == '\r' || *p == '#') break;
                    char* end = nullptr;
                    const long i = std::strtol(p, &end, 10);
                    if (end == p) break;
                    face.push_back(i > 0 ? static_cast<int>(i - 1) : nv + static_cast<int>(i));
                    p = end;
                    while (*p && *p != ' ' && *p != '\t') ++p;  // skip /vt/vn
                }
                for (size_t k = 2; k < face.size(); ++k) {  // fan: (0, k-1, k)
                    for (int c : {face[0], face[k - 1], face[k]}) {
                        index_t idx;
                        idx.vertex_index = c;
                        shape.mesh.indices.push_back(idx);
                    }
                    shape.mesh.num_face_vertices.push_back(3);
                    shape.mesh.material_ids.push_back(-1);
                    shape.mesh.smoothing_group_ids.push_back(0);
                }
            }
        }
        if (!shape.mesh.indices.empty()) shapes_.push_back(std::move(shape));
        valid_ = true;
        return true;
    }

    bool Valid() const { return valid_; }
    const std::string& Error() const { return error_; }
    const std::string& Warning() const { return warning_; }
    const attrib_t& GetAttrib() const { return attrib_; }
    const std::vector<shape_t>& GetShapes() const { return shapes_; }
    const std::vector<material_t>& GetMaterials() const { return materials_; }

private:
    bool valid_ = false;
    std::string error_, warning_;
    attrib_t attrib_;
    std::vector<shape_t> shapes_;
    std::vector<material_t> materials_;
};

}  // namespace tinyobj
