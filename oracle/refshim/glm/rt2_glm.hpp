// rt2_glm.hpp — stand-in for the part of glm that the reference's src/cpu_raytrace names (SURVEY.md
// Appendix C). TEST INFRASTRUCTURE ONLY: the reference build (oracle/Makefile, target ref) compiles the
// reference's sources against this header because glm itself is not available.
//
// Every function evaluates in glm's published operation order (glm 0.9.9 / 1.0, the scalar paths):
//   dot(vec3)       tmp = a * b; (tmp.x + tmp.y) + tmp.z
//   normalize       v * inversesqrt(dot(v, v)), inversesqrt(x) = 1 / sqrt(x)
//   length          sqrt(dot(v, v))
//   min / max       min(x, y) = (y < x) ? y : x ; max(x, y) = (x < y) ? y : x
//   mat4 * vec4     (m0 * v.x + m1 * v.y) + (m2 * v.z + m3 * v.w)
//   mat3 * vec3     row sums left to right
//   mat4 * mat4     ((A0 * b0 + A1 * b1) + A2 * b2) + A3 * b3 per column
//   inverse(mat4)   the cofactor form with one division (1 / determinant)
//   pow, sqrt, acos, tan, sin, cos   the std:: ones (glm pulls them in by using-declarations), so
//                   pow(float, int) promotes to double
// This is a restatement of glm and is compared with nothing but the oracle's own restatement.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace glm {

using std::acos;
using std::cos;
using std::pow;
using std::sin;
using std::sqrt;
using std::tan;

template <int L, typename T>
struct vec;

template <typename T>
struct vec<2, T> {
  T x, y;
  constexpr vec() : x(0), y(0) {}
  constexpr explicit vec(T s) : x(s), y(s) {}
  template <typename X, typename Y>
  constexpr vec(X x_, Y y_) : x(static_cast<T>(x_)), y(static_cast<T>(y_)) {}
  template <typename U>
  constexpr vec(const vec<2, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)) {}
  T& operator[](int i) { return i == 0 ? x : y; }
  const T& operator[](int i) const { return i == 0 ? x : y; }
};

template <typename T>
struct vec<3, T> {
  T x, y, z;
  constexpr vec() : x(0), y(0), z(0) {}
  constexpr explicit vec(T s) : x(s), y(s), z(s) {}
  template <typename X, typename Y, typename Z>
  constexpr vec(X x_, Y y_, Z z_) : x(static_cast<T>(x_)), y(static_cast<T>(y_)), z(static_cast<T>(z_)) {}
  template <typename U>
  constexpr vec(const vec<3, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}
  template <typename U>
  constexpr explicit vec(const vec<4, U>& v);
  T& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
  const T& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
  vec& operator+=(const vec& o) {
    x += o.x;
    y += o.y;
    z += o.z;
    return *this;
  }
  vec& operator-=(const vec& o) {
    x -= o.x;
    y -= o.y;
    z -= o.z;
    return *this;
  }
  template <typename U>
  vec& operator*=(U s) {
    x *= static_cast<T>(s);
    y *= static_cast<T>(s);
    z *= static_cast<T>(s);
    return *this;
  }
  template <typename U>
  vec& operator/=(U s) {
    x /= static_cast<T>(s);
    y /= static_cast<T>(s);
    z /= static_cast<T>(s);
    return *this;
  }
};

template <typename T>
struct vec<4, T> {
  T x, y, z, w;
  constexpr vec() : x(0), y(0), z(0), w(0) {}
  constexpr explicit vec(T s) : x(s), y(s), z(s), w(s) {}
  template <typename X, typename Y, typename Z, typename W>
  constexpr vec(X x_, Y y_, Z z_, W w_)
      : x(static_cast<T>(x_)), y(static_cast<T>(y_)), z(static_cast<T>(z_)), w(static_cast<T>(w_)) {}
  template <typename U, typename W>
  constexpr vec(const vec<3, U>& v, W w_)
      : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)), w(static_cast<T>(w_)) {}
  T& operator[](int i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
  const T& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
};

template <typename T>
template <typename U>
constexpr vec<3, T>::vec(const vec<4, U>& v)
    : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}

// component-wise arithmetic
template <typename T>
vec<3, T> operator+(const vec<3, T>& a, const vec<3, T>& b) {
  return {a.x + b.x, a.y + b.y, a.z + b.z};
}
template <typename T>
vec<3, T> operator-(const vec<3, T>& a, const vec<3, T>& b) {
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
template <typename T>
vec<3, T> operator*(const vec<3, T>& a, const vec<3, T>& b) {
  return {a.x * b.x, a.y * b.y, a.z * b.z};
}
template <typename T>
vec<3, T> operator*(const vec<3, T>& a, T s) {
  return {a.x * s, a.y * s, a.z * s};
}
template <typename T>
vec<3, T> operator*(T s, const vec<3, T>& a) {
  return {s * a.x, s * a.y, s * a.z};
}
template <typename T>
vec<3, T> operator/(const vec<3, T>& a, T s) {
  return {a.x / s, a.y / s, a.z / s};
}
template <typename T>
vec<3, T> operator-(const vec<3, T>& a) {
  return {-a.x, -a.y, -a.z};
}
template <typename T>
vec<4, T> operator+(const vec<4, T>& a, const vec<4, T>& b) {
  return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
}
template <typename T>
vec<4, T> operator-(const vec<4, T>& a, const vec<4, T>& b) {
  return {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
}
template <typename T>
vec<4, T> operator*(const vec<4, T>& a, const vec<4, T>& b) {
  return {a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w};
}
template <typename T>
vec<4, T> operator*(const vec<4, T>& a, T s) {
  return {a.x * s, a.y * s, a.z * s, a.w * s};
}

// geometric
template <typename T>
T dot(const vec<3, T>& a, const vec<3, T>& b) {
  vec<3, T> tmp(a * b);
  return (tmp.x + tmp.y) + tmp.z;
}
template <typename T>
vec<3, T> cross(const vec<3, T>& x, const vec<3, T>& y) {
  return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y};
}
template <typename T>
T inversesqrt(T x) {
  return static_cast<T>(1) / std::sqrt(x);
}
template <typename T>
vec<3, T> normalize(const vec<3, T>& v) {
  return v * inversesqrt(dot(v, v));
}
template <typename T>
T length(const vec<3, T>& v) {
  return std::sqrt(dot(v, v));
}

// common
template <typename T>
constexpr T min(T x, T y) {
  return (y < x) ? y : x;
}
template <typename T>
constexpr T max(T x, T y) {
  return (x < y) ? y : x;
}
template <typename T>
vec<3, T> floor(const vec<3, T>& v) {
  return {std::floor(v.x), std::floor(v.y), std::floor(v.z)};
}
template <typename T>
vec<3, T> clamp(const vec<3, T>& v, T lo, T hi) {
  return {min(max(v.x, lo), hi), min(max(v.y, lo), hi), min(max(v.z, lo), hi)};
}
template <typename T>
constexpr T radians(T degrees) {
  return degrees * static_cast<T>(0.01745329251994329576923690768489);
}

// matrices, column-major: m[column][row]
template <int C, int R, typename T>
struct mat;

template <typename T>
struct mat<4, 4, T> {
  vec<4, T> value[4];
  constexpr mat() = default;
  constexpr explicit mat(T s) : value{{s, 0, 0, 0}, {0, s, 0, 0}, {0, 0, s, 0}, {0, 0, 0, s}} {}
  vec<4, T>& operator[](int i) { return value[i]; }
  const vec<4, T>& operator[](int i) const { return value[i]; }
};

template <typename T>
struct mat<3, 3, T> {
  vec<3, T> value[3];
  constexpr mat() = default;
  constexpr explicit mat(T s) : value{{s, 0, 0}, {0, s, 0}, {0, 0, s}} {}
  constexpr mat(const mat<4, 4, T>& m) : value{vec<3, T>(m[0]), vec<3, T>(m[1]), vec<3, T>(m[2])} {}
  vec<3, T>& operator[](int i) { return value[i]; }
  const vec<3, T>& operator[](int i) const { return value[i]; }
};

template <typename T>
vec<4, T> operator*(const mat<4, 4, T>& m, const vec<4, T>& v) {
  const vec<4, T> Mul0 = m[0] * v.x, Mul1 = m[1] * v.y;
  const vec<4, T> Add0 = Mul0 + Mul1;
  const vec<4, T> Mul2 = m[2] * v.z, Mul3 = m[3] * v.w;
  const vec<4, T> Add1 = Mul2 + Mul3;
  return Add0 + Add1;
}
template <typename T>
vec<3, T> operator*(const mat<3, 3, T>& m, const vec<3, T>& v) {
  return {m[0][0] * v.x + m[1][0] * v.y + m[2][0] * v.z, m[0][1] * v.x + m[1][1] * v.y + m[2][1] * v.z,
          m[0][2] * v.x + m[1][2] * v.y + m[2][2] * v.z};
}
template <typename T>
mat<4, 4, T> operator*(const mat<4, 4, T>& a, const mat<4, 4, T>& b) {
  mat<4, 4, T> r;
  for (int i = 0; i < 4; i++) r[i] = ((a[0] * b[i][0] + a[1] * b[i][1]) + a[2] * b[i][2]) + a[3] * b[i][3];
  return r;
}
template <typename T>
mat<4, 4, T> transpose(const mat<4, 4, T>& m) {
  mat<4, 4, T> r;
  for (int c = 0; c < 4; c++)
    for (int w = 0; w < 4; w++) r[c][w] = m[w][c];
  return r;
}
template <typename T>
mat<4, 4, T> inverse(const mat<4, 4, T>& m) {
  using V = vec<4, T>;
  T Coef00 = m[2][2] * m[3][3] - m[3][2] * m[2][3];
  T Coef02 = m[1][2] * m[3][3] - m[3][2] * m[1][3];
  T Coef03 = m[1][2] * m[2][3] - m[2][2] * m[1][3];
  T Coef04 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
  T Coef06 = m[1][1] * m[3][3] - m[3][1] * m[1][3];
  T Coef07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
  T Coef08 = m[2][1] * m[3][2] - m[3][1] * m[2][2];
  T Coef10 = m[1][1] * m[3][2] - m[3][1] * m[1][2];
  T Coef11 = m[1][1] * m[2][2] - m[2][1] * m[1][2];
  T Coef12 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
  T Coef14 = m[1][0] * m[3][3] - m[3][0] * m[1][3];
  T Coef15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
  T Coef16 = m[2][0] * m[3][2] - m[3][0] * m[2][2];
  T Coef18 = m[1][0] * m[3][2] - m[3][0] * m[1][2];
  T Coef19 = m[1][0] * m[2][2] - m[2][0] * m[1][2];
  T Coef20 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
  T Coef22 = m[1][0] * m[3][1] - m[3][0] * m[1][1];
  T Coef23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
  V Fac0(Coef00, Coef00, Coef02, Coef03);
  V Fac1(Coef04, Coef04, Coef06, Coef07);
  V Fac2(Coef08, Coef08, Coef10, Coef11);
  V Fac3(Coef12, Coef12, Coef14, Coef15);
  V Fac4(Coef16, Coef16, Coef18, Coef19);
  V Fac5(Coef20, Coef20, Coef22, Coef23);
  V Vec0(m[1][0], m[0][0], m[0][0], m[0][0]);
  V Vec1(m[1][1], m[0][1], m[0][1], m[0][1]);
  V Vec2(m[1][2], m[0][2], m[0][2], m[0][2]);
  V Vec3(m[1][3], m[0][3], m[0][3], m[0][3]);
  V Inv0(Vec1 * Fac0 - Vec2 * Fac1 + Vec3 * Fac2);
  V Inv1(Vec0 * Fac0 - Vec2 * Fac3 + Vec3 * Fac4);
  V Inv2(Vec0 * Fac1 - Vec1 * Fac3 + Vec3 * Fac5);
  V Inv3(Vec0 * Fac2 - Vec1 * Fac4 + Vec2 * Fac5);
  V SignA(+1, -1, +1, -1);
  V SignB(-1, +1, -1, +1);
  mat<4, 4, T> Inverse;
  Inverse[0] = Inv0 * SignA;
  Inverse[1] = Inv1 * SignB;
  Inverse[2] = Inv2 * SignA;
  Inverse[3] = Inv3 * SignB;
  V Row0(Inverse[0][0], Inverse[1][0], Inverse[2][0], Inverse[3][0]);
  V Dot0(m[0] * Row0);
  T Dot1 = (Dot0.x + Dot0.y) + (Dot0.z + Dot0.w);
  T OneOverDeterminant = static_cast<T>(1) / Dot1;
  for (int i = 0; i < 4; i++) Inverse[i] = Inverse[i] * OneOverDeterminant;
  return Inverse;
}

// transforms (matrix_transform.inl) and quaternions (quaternion.inl: angleAxis, mat3_cast)
template <typename T>
mat<4, 4, T> translate(const mat<4, 4, T>& m, const vec<3, T>& v) {
  mat<4, 4, T> r(m);
  r[3] = ((m[0] * v[0] + m[1] * v[1]) + m[2] * v[2]) + m[3];
  return r;
}
template <typename T>
mat<4, 4, T> scale(const mat<4, 4, T>& m, const vec<3, T>& v) {
  mat<4, 4, T> r;
  r[0] = m[0] * v[0];
  r[1] = m[1] * v[1];
  r[2] = m[2] * v[2];
  r[3] = m[3];
  return r;
}
template <typename T>
struct qua {
  T w, x, y, z;
  constexpr qua() : w(1), x(0), y(0), z(0) {}  // glm leaves it uninitialised; the identity is this project's choice
  constexpr qua(T w_, T x_, T y_, T z_) : w(w_), x(x_), y(y_), z(z_) {}
};
template <typename T>
qua<T> angleAxis(T angle, const vec<3, T>& v) {
  const T a(angle);
  const T s = std::sin(a * static_cast<T>(0.5));
  const vec<3, T> vs = v * s;
  return qua<T>(std::cos(a * static_cast<T>(0.5)), vs.x, vs.y, vs.z);
}
template <typename T>
mat<4, 4, T> toMat4(const qua<T>& q) {
  mat<4, 4, T> R(T(1));
  T qxx(q.x * q.x), qyy(q.y * q.y), qzz(q.z * q.z), qxz(q.x * q.z), qxy(q.x * q.y), qyz(q.y * q.z);
  T qwx(q.w * q.x), qwy(q.w * q.y), qwz(q.w * q.z);
  R[0][0] = T(1) - T(2) * (qyy + qzz);
  R[0][1] = T(2) * (qxy + qwz);
  R[0][2] = T(2) * (qxz - qwy);
  R[1][0] = T(2) * (qxy - qwz);
  R[1][1] = T(1) - T(2) * (qxx + qzz);
  R[1][2] = T(2) * (qyz + qwx);
  R[2][0] = T(2) * (qxz + qwy);
  R[2][1] = T(2) * (qyz - qwx);
  R[2][2] = T(1) - T(2) * (qxx + qyy);
  return R;
}

using vec2 = vec<2, float>;
using vec3 = vec<3, float>;
using vec4 = vec<4, float>;
using dvec2 = vec<2, double>;
using dvec3 = vec<3, double>;
using dvec4 = vec<4, double>;
using ivec2 = vec<2, int>;
using ivec3 = vec<3, int>;
using u8vec4 = vec<4, std::uint8_t>;
using mat3 = mat<3, 3, float>;
using mat4 = mat<4, 4, float>;
using dmat3 = mat<3, 3, double>;
using dmat4 = mat<4, 4, double>;
using quat = qua<float>;
using dquat = qua<double>;

}  // namespace glm
