// Stand-in for <glm/glm.hpp>, written for this project: only what the reference's voxelizer files
// (VoxelBuilder.hpp, voxelgrid*.{hpp,cpp}, octTree.hpp, common/obj_loader.h, shaders/host_device.h) use.
// Every operation follows glm's own scalar definition (glm/detail/func_common.inl, func_geometric.inl,
// type_vec3.inl, GLM_FORCE_PURE semantics): component-wise, no SIMD, no fused multiply-add.
#pragma once

#include <cstddef>
#include <cstdint>  // glm/detail/setup.hpp includes it; shaders/host_device.h relies on it for uint64_t

namespace glm {

template <typename T>
struct tvec2 {
    T x, y;
    constexpr tvec2() = default;
    template <typename X, typename Y>
    constexpr tvec2(X a, Y b) : x(static_cast<T>(a)), y(static_cast<T>(b)) {}
};

template <typename T>
struct tvec3 {
    T x, y, z;
    // glm's default constructor leaves the components uninitialised (no GLM_FORCE_CTOR_INIT); value-initialisation zeroes
    constexpr tvec3() = default;
    constexpr explicit tvec3(T s) : x(s), y(s), z(s) {}
    // vec(X x, Y y, Z z): each component static_cast to T (type_vec3.inl)
    template <typename X, typename Y, typename Z>
    constexpr tvec3(X a, Y b, Z c) : x(static_cast<T>(a)), y(static_cast<T>(b)), z(static_cast<T>(c)) {}
    // explicit vec(vec<3, U> const&): converting constructor
    template <typename U>
    constexpr explicit tvec3(const tvec3<U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}
};

template <typename T>
struct tvec4 {
    T x, y, z, w;
    constexpr tvec4() = default;
    template <typename X, typename Y, typename Z, typename W>
    constexpr tvec4(X a, Y b, Z c, W d) : x(static_cast<T>(a)), y(static_cast<T>(b)), z(static_cast<T>(c)), w(static_cast<T>(d)) {}
};

struct mat4 {
    tvec4<float> value[4];
};

using vec2 = tvec2<float>;
using vec3 = tvec3<float>;
using vec4 = tvec4<float>;
using ivec3 = tvec3<int>;
using uvec3 = tvec3<unsigned int>;
using bvec3 = tvec3<bool>;

// operator== (type_vec3.inl): component-wise ==, so -0 == +0 and NaN != NaN
template <typename T>
constexpr bool operator==(const tvec3<T>& a, const tvec3<T>& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
template <typename T>
constexpr bool operator!=(const tvec3<T>& a, const tvec3<T>& b) { return !(a == b); }

// Arithmetic operators (type_vec3.inl): one scalar operation per component, vec/vec and vec/scalar both ways
#define VXREF_GLM_BINOP(op)                                                                                              \
    template <typename T>                                                                                               \
    constexpr tvec3<T> operator op(const tvec3<T>& a, const tvec3<T>& b) { return tvec3<T>(a.x op b.x, a.y op b.y, a.z op b.z); } \
    template <typename T>                                                                                               \
    constexpr tvec3<T> operator op(const tvec3<T>& a, T s) { return tvec3<T>(a.x op s, a.y op s, a.z op s); }           \
    template <typename T>                                                                                               \
    constexpr tvec3<T> operator op(T s, const tvec3<T>& a) { return tvec3<T>(s op a.x, s op a.y, s op a.z); }
VXREF_GLM_BINOP(+)
VXREF_GLM_BINOP(-)
VXREF_GLM_BINOP(*)
#undef VXREF_GLM_BINOP

template <typename T>
constexpr tvec3<T> operator-(const tvec3<T>& a) { return tvec3<T>(-a.x, -a.y, -a.z); }

// min(x, y) = (y < x) ? y : x and max(x, y) = (x < y) ? y : x (func_common.inl): on a -0 / +0 tie both return x
template <typename T>
constexpr T min(T x, T y) { return (y < x) ? y : x; }
template <typename T>
constexpr T max(T x, T y) { return (x < y) ? y : x; }
template <typename T>
constexpr tvec3<T> min(const tvec3<T>& a, const tvec3<T>& b) { return tvec3<T>(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
template <typename T>
constexpr tvec3<T> max(const tvec3<T>& a, const tvec3<T>& b) { return tvec3<T>(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }

// abs (compute_abs<genFIType, true>, func_common.inl): x >= 0 ? x : -x, so abs(-0) is -0
template <typename T>
constexpr T abs(T x) { return x >= T(0) ? x : -x; }
template <typename T>
constexpr tvec3<T> abs(const tvec3<T>& a) { return tvec3<T>(abs(a.x), abs(a.y), abs(a.z)); }

// dot (compute_dot<vec<3>>, func_geometric.inl): tmp = a * b; return tmp.x + tmp.y + tmp.z, i.e. (x + y) + z
template <typename T>
constexpr T dot(const tvec3<T>& a, const tvec3<T>& b)
{
    const tvec3<T> tmp(a * b);
    return tmp.x + tmp.y + tmp.z;
}

// cross (compute_cross, func_geometric.inl): (x.y*y.z - y.y*x.z, x.z*y.x - y.z*x.x, x.x*y.y - y.x*x.y)
template <typename T>
constexpr tvec3<T> cross(const tvec3<T>& x, const tvec3<T>& y)
{
    return tvec3<T>(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}

// lessThanEqual / all (vector_relational.inl)
template <typename T>
constexpr bvec3 lessThanEqual(const tvec3<T>& a, const tvec3<T>& b) { return bvec3(a.x <= b.x, a.y <= b.y, a.z <= b.z); }
constexpr bool all(const bvec3& v) { return v.x && v.y && v.z; }

}  // namespace glm
