// ref_driver.cpp — C ABI over the reference's own compiled src/cpu_raytrace (oracle/Makefile, target ref;
// loaded by tests/test_reference_build.py and tests/golden/make_ref_golden.py through ctypes).
// TEST INFRASTRUCTURE ONLY; never on the GPU machine's path and never the product path.
//
// What is the reference's own code here: every Hit, the BVH build, the camera, the materials, the textures,
// the Perlin tables and RayTracer::Update (with RayColor inside it). What is restated here:
//   * the scene loader, written from Serialize.cpp:106-360 over the project's csrc/json.h (the reference's
//     needs nlohmann::json): same order of textures, materials, implicit appends, primitives and nodes; a
//     missing "rotation" is the identity quaternion (the reference leaves it uninitialised); plus the
//     project's legacy-schema adapter (primitives given as {"spheres", "quads", "boxes"}, camera by file
//     name next to the scene), which the reference's loader does not have;
//   * the BVH wrap of App.cpp:126;
//   * RandReal()'s generator: ref_prelude.hpp routes it to rt2_ref_uniform() below, a Philox4x32-10 stream
//     with the oracle's keying (counter (a, b, block, tag), key = seed, u = (word >> 8) * 2^-24).
// ref_render drives RayTracer::Update one pixel and one frame at a time (iter_ holds one entry, frame_idx_
// is set before the call) and re-keys the stream to (seed, pixel, frame) before each call.
#define private public  // iter_, frame_idx_, accumulation_data_ of RayTracer; the camera's derived values
#include "cpu_raytrace/RayTracer.hpp"
#include "cpu_raytrace/Scene.hpp"
#undef private
#include "cpu_raytrace/ConstantMedium.hpp"
#include "cpu_raytrace/HitRecord.hpp"
#include "cpu_raytrace/Material.hpp"
#include "cpu_raytrace/Quad.hpp"
#include "cpu_raytrace/Texture.hpp"
#include "cpu_raytrace/Transform.hpp"

#include <cstdlib>

#include "json.h"

void HandleAssert(const char* msg, const char* condition, const char* filename, uint64_t line) {
  std::cerr << msg << ": " << condition << " at " << filename << ":" << line << '\n';
}

namespace {

using rt2::Json;
namespace cpu = raytrace2::cpu;

// ---- the uniform hook: Philox4x32-10 (Salmon et al., SC'11) ---------------------------------------------
constexpr uint32_t kTagPath = 0x52543250u;    // "RT2P"
constexpr uint32_t kTagPerlin = 0x52543254u;  // "RT2T"

struct Stream {
  uint32_t k0{0}, k1{0}, a{0}, b{0}, tag{kTagPath}, block{0};
  uint32_t buf[4]{};
  int idx{4};
  uint64_t draws{0};
};
Stream g_stream;

void Philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

void Rekey(uint64_t seed, uint32_t a, uint32_t b, uint32_t tag) {
  g_stream = Stream{};
  g_stream.k0 = (uint32_t)seed;
  g_stream.k1 = (uint32_t)(seed >> 32);
  g_stream.a = a;
  g_stream.b = b;
  g_stream.tag = tag;
}

// ---- the loader -----------------------------------------------------------------------------------------
std::string g_err;

double Num(const Json& o, const char* key, double dflt) {
  const Json* v = o.find(key);
  return (v && (v->is_number() || v->is_bool())) ? v->as_number() : dflt;
}
bool Vec3At(const Json& o, const char* key, vec3& out) {
  const Json* v = o.find(key);
  if (!v || !v->is_array() || v->items().size() < 3) return false;
  out = vec3{static_cast<real>(v->items()[0].as_number()), static_cast<real>(v->items()[1].as_number()),
             static_cast<real>(v->items()[2].as_number())};
  return true;
}
vec3 Vec3Or(const Json& o, const char* key, vec3 dflt) {
  Vec3At(o, key, dflt);
  return dflt;
}
std::string Str(const Json& o, const char* key) {
  const Json* v = o.find(key);
  return (v && v->is_string()) ? v->as_string() : std::string();
}

// Serialize.cpp:32-40
cpu::Camera LoadCamera(const Json& o) {
  cpu::Camera cam;
  cam.SetFOV(static_cast<real>(static_cast<int>(Num(o, "fov", 90))));
  cam.SetCenter(Vec3Or(o, "center", vec3{0, 0, 1}));
  cam.SetLookAt(Vec3Or(o, "look_at", vec3{0, 0, 0}));
  cam.SetDefocusAngle(static_cast<real>(Num(o, "defocus_angle", 0.0)));
  cam.SetFocusDistance(static_cast<real>(Num(o, "focus_distance", 1.0)));
  return cam;
}

// Serialize.cpp:106-132
std::optional<mat4> ParseTransform(const Json& node) {
  const Json* t = node.find("transform");
  if (!t || !t->is_object()) return std::nullopt;
  const vec3 translation = Vec3Or(*t, "translation", vec3{0});
  quat rotation;  // the identity when "rotation" is absent
  const Json* r = t->find("rotation");
  if (r && r->is_array() && r->items().size() >= 4) {
    const real angle = static_cast<real>(r->items()[0].as_number());
    const vec3 axis{static_cast<real>(r->items()[1].as_number()), static_cast<real>(r->items()[2].as_number()),
                    static_cast<real>(r->items()[3].as_number())};
    rotation = glm::angleAxis(glm::radians(angle), axis);
  }
  const vec3 scale = Vec3Or(*t, "scale", vec3{1});
  return glm::translate(mat4(1), translation) * glm::toMat4(rotation) * glm::scale(mat4(1), scale);
}

// Serialize.cpp:161-197
std::shared_ptr<cpu::Hittable> ParseNode(std::vector<std::shared_ptr<cpu::Hittable>>& list, const Json& node) {
  std::shared_ptr<cpu::Hittable> ret;
  if (node.contains("primitive")) {
    const int idx = static_cast<int>(Num(node, "primitive", -1));
    if (idx < 0 || idx >= static_cast<int>(list.size())) {
      g_err = "primitive out of range of primitives";
      return nullptr;
    }
    ret = list[static_cast<size_t>(idx)];
  }
  const auto transform = ParseTransform(node);
  if (const Json* children = node.find("children")) {
    if (!children->is_array()) {
      g_err = "children entry must be an array";
      return nullptr;
    }
    auto children_list = std::make_shared<cpu::HittableList>();
    if (ret) children_list->Add(ret);
    for (const Json& child : children->items()) {
      auto h = ParseNode(list, child);
      if (!h) return nullptr;
      children_list->Add(h);
    }
    ret = children_list;
  }
  if (!ret) {
    g_err = "error parsing node";
    return nullptr;
  }
  if (transform.has_value()) return std::make_shared<cpu::TransformedHittable>(ret, transform.value());
  return ret;
}

struct RefScene {
  cpu::Scene scene;
  uint64_t seed{0};
};

// A material or texture that reads a texture index past the table would read out of bounds in Value().
bool CheckIndices(const cpu::Scene& s) {
  for (const auto& m : s.materials) {
    uint32_t idx = 0;
    bool reads = true;
    if (auto* t = std::get_if<cpu::MaterialTexture>(&m)) idx = t->tex_idx;
    else if (auto* l = std::get_if<cpu::DiffuseLight>(&m)) idx = l->tex_idx;
    else if (auto* i = std::get_if<cpu::MaterialIsotropic>(&m)) idx = i->tex_idx;
    else reads = false;
    if (reads && idx >= s.textures.size()) return false;
  }
  for (const auto& t : s.textures)
    if (auto* c = std::get_if<cpu::texture::Checker>(&t))
      if (c->even_tex_idx >= s.textures.size() || c->odd_tex_idx >= s.textures.size()) return false;
  return true;
}

// Serialize.cpp:199-360, then App.cpp:126
RefScene* LoadScene(const std::string& path, uint64_t seed) {
  Json obj;
  if (!Json::ParseFile(path, obj, g_err)) return nullptr;
  auto rs = std::make_unique<RefScene>();
  rs->seed = seed;
  cpu::Scene& scene = rs->scene;
  const std::string dir = path.substr(0, path.find_last_of('/') + 1);

  const Json* cam = obj.find("camera");
  scene.background_color = Vec3Or(obj, "background_color", vec3{1, 1, 1});
  if (cam && cam->is_object()) {
    scene.cam = LoadCamera(*cam);
  } else {  // a camera file next to the scene; "cam1" when the scene names none (legacy adapter)
    const std::string name = (cam && cam->is_string()) ? cam->as_string() : std::string("cam1");
    Json cj;
    if (!Json::ParseFile(dir + name + ".json", cj, g_err)) return nullptr;
    scene.cam = LoadCamera(cj);
    scene.cam_name = name + ".json";
  }

  uint32_t noise_ordinal = 0;
  const Json* textures = obj.find("textures");
  if (textures && textures->is_array()) {
    for (const Json& t : textures->items()) {
      const std::string type = Str(t, "type");
      cpu::texture::TextureVariant tex;
      if (type == "solid_color") {
        tex = cpu::texture::SolidColor{.albedo = Vec3Or(t, "albedo", vec3{1, 1, 1})};
      } else if (type == "checker") {
        tex = cpu::texture::Checker{static_cast<real>(Num(t, "scale", 1.0)),
                                    static_cast<uint32_t>(Num(t, "even_tex_idx", 0)),
                                    static_cast<uint32_t>(Num(t, "odd_tex_idx", 0))};
      } else if (type == "noise") {
        // the tables are drawn inside PerlinNoiseGen's constructor: key the stream for this texture
        Rekey(seed, noise_ordinal++, 0xFFFFFFFFu, kTagPerlin);
        tex = cpu::texture::Noise{
            .noise = cpu::PerlinNoiseGen{static_cast<int>(Num(t, "point_count", 256))},
            .albedo = Vec3Or(t, "albedo", vec3{1, 1, 1}),
            .scale = static_cast<real>(Num(t, "scale", 1.0)),
            .noise_type = static_cast<cpu::texture::NoiseType>(
                static_cast<int>(Num(t, "noise_type", static_cast<int>(cpu::texture::NoiseType::kMarble))))};
      } else {
        g_err = "Invalid texture type: " + type;
        return nullptr;
      }
      scene.textures.emplace_back(tex);
    }
  }

  const Json* materials = obj.find("materials");
  if (materials && materials->is_array()) {
    for (const Json& m : materials->items()) {
      const std::string type = Str(m, "type");
      if (type.empty()) {
        g_err = "material type field empty";
        return nullptr;
      }
      cpu::MaterialVariant mat;
      if (type == "lambertian") {
        mat = cpu::MaterialLambertian{.albedo = Vec3Or(m, "albedo", vec3{1, 1, 1})};
      } else if (type == "dielectric") {
        mat = cpu::MaterialDielectric{.refraction_index = static_cast<real>(Num(m, "refraction_index", 1.0))};
      } else if (type == "metal") {
        mat = cpu::MaterialMetal{.albedo = Vec3Or(m, "albedo", vec3{1, 1, 1}),
                                 .fuzz = static_cast<real>(Num(m, "fuzz", 0.0))};
      } else if (type == "texture" || type == "diffuse_light") {
        uint32_t tex_idx;
        if (m.contains("tex_idx")) {
          tex_idx = static_cast<uint32_t>(Num(m, "tex_idx", 0));
        } else if (m.contains("albedo")) {
          tex_idx = static_cast<uint32_t>(scene.textures.size());
          scene.textures.emplace_back(cpu::texture::SolidColor{.albedo = Vec3Or(m, "albedo", vec3{1, 1, 1})});
        } else {
          g_err = "invalid " + type + ", must contain tex_idx or albedo";
          return nullptr;
        }
        if (type == "texture") {
          mat = cpu::MaterialTexture{.tex_idx = tex_idx};
        } else {
          mat = cpu::DiffuseLight{.tex_idx = tex_idx};
        }
      } else {
        g_err = "Invalid material type";
        return nullptr;
      }
      scene.materials.emplace_back(mat);
    }
  }

  std::vector<std::shared_ptr<cpu::Hittable>> list;
  const Json* prims = obj.find("primitives");
  if (prims && prims->is_object()) {
    // legacy schema: one scene node per primitive, the groups in file order, each in array order
    for (const auto& group : prims->members()) {
      for (const Json& p : group.second.items()) {
        const auto mat = static_cast<uint32_t>(Num(p, "material_id", 0));
        std::shared_ptr<cpu::Hittable> h;
        if (group.first == "spheres") {
          h = std::make_shared<cpu::Sphere>(Vec3Or(p, "center", vec3{0, 0, 0}), Vec3Or(p, "displacement", vec3{0, 0, 0}),
                                            static_cast<real>(Num(p, "radius", 0.5)), mat);
        } else if (group.first == "quads") {
          h = std::make_shared<cpu::Quad>(Vec3Or(p, "q", vec3{0, 0, 0}), Vec3Or(p, "u", vec3{1, 0, 0}),
                                          Vec3Or(p, "v", vec3{0, 0, 1}), mat);
        } else if (group.first == "boxes") {
          h = std::make_shared<cpu::HittableList>(
              cpu::MakeBox(Vec3Or(p, "a", vec3{0, 0, 0}), Vec3Or(p, "b", vec3{1, 1, 1}), mat));
        } else {
          g_err = "legacy primitives: unknown group " + group.first;
          return nullptr;
        }
        scene.hittable_list.Add(h);
      }
    }
  } else if (prims && prims->is_array()) {
    for (const Json& p : prims->items()) {
      const std::string type = Str(p, "type");
      const auto mat = static_cast<uint32_t>(Num(p, "material", 0));
      std::shared_ptr<cpu::Hittable> hittable;
      if (type == "quad") {
        hittable = std::make_shared<cpu::Quad>(Vec3Or(p, "q", vec3{0, 0, 0}), Vec3Or(p, "u", vec3{1, 0, 0}),
                                               Vec3Or(p, "v", vec3{0, 0, 1}), mat);
      } else if (type == "box") {
        hittable = std::make_shared<cpu::HittableList>(
            cpu::MakeBox(Vec3Or(p, "a", vec3{0, 0, 0}), Vec3Or(p, "b", vec3{1, 1, 1}), mat));
      } else if (type == "sphere") {
        hittable = std::make_shared<cpu::Sphere>(Vec3Or(p, "center", vec3{0, 0, 0}),
                                                 Vec3Or(p, "displacement", vec3{0, 0, 0}),
                                                 static_cast<real>(Num(p, "radius", 0.5)), mat);
      } else {
        continue;  // "invalid primitive type"
      }
      if (const Json* cm = p.find("constant_medium")) {
        uint32_t material_idx;
        if (cm->contains("albedo")) {
          auto iso = cpu::MaterialIsotropic{.tex_idx = static_cast<uint32_t>(scene.textures.size())};
          scene.textures.emplace_back(cpu::texture::SolidColor{.albedo = Vec3Or(*cm, "albedo", vec3{0, 0, 0})});
          material_idx = static_cast<uint32_t>(scene.materials.size());
          scene.materials.emplace_back(iso);
        } else if (cm->contains("material")) {
          material_idx = static_cast<uint32_t>(Num(*cm, "material", 0));
        } else {
          continue;  // "constant_medium must contain 'albedo' or 'material'"
        }
        const real density = static_cast<real>(Num(*cm, "density", 0.01));
        hittable = std::make_shared<cpu::ConstantMedium>(hittable, density, material_idx);
      }
      list.emplace_back(hittable);
    }
    const Json* nodes = obj.find("scene");
    if (nodes && nodes->is_array()) {
      for (const Json& n : nodes->items()) {
        auto h = ParseNode(list, n);
        if (!h) return nullptr;
        scene.hittable_list.Add(h);
      }
    }
  }
  if (scene.hittable_list.objects.empty()) {
    g_err = "scene has no objects";
    return nullptr;
  }
  if (!CheckIndices(scene)) {
    g_err = "material texture index out of range";
    return nullptr;
  }
  // App.cpp:126
  scene.hittable_list = cpu::HittableList{std::make_shared<cpu::BVHNode>(scene.hittable_list)};
  return rs.release();
}

}  // namespace

extern "C" {

float rt2_ref_uniform() {
  Stream& s = g_stream;
  if (s.idx == 4) {
    s.buf[0] = s.a;
    s.buf[1] = s.b;
    s.buf[2] = s.block++;
    s.buf[3] = s.tag;
    Philox(s.buf, s.k0, s.k1);
    s.idx = 0;
  }
  s.draws++;
  return static_cast<float>(s.buf[s.idx++] >> 8) * (1.0f / 16777216.0f);
}

const char* ref_last_error() { return g_err.c_str(); }

void* ref_scene_load(const char* path, uint64_t seed) { return LoadScene(path, seed); }
void ref_scene_free(void* sp) { delete static_cast<RefScene*>(sp); }

// n_materials, n_textures, then per texture (up to cap): 0 solid, 1 checker, 2 noise
int ref_scene_info(void* sp, int* n_materials, int* tex_kinds, int cap) {
  const cpu::Scene& s = static_cast<RefScene*>(sp)->scene;
  *n_materials = static_cast<int>(s.materials.size());
  for (size_t i = 0; i < s.textures.size() && static_cast<int>(i) < cap; i++) tex_kinds[i] = static_cast<int>(s.textures[i].index());
  return static_cast<int>(s.textures.size());
}

// The first n uniforms of the path stream of (seed, pixel, frame), through the hook RandReal() calls.
void ref_uniforms(uint64_t seed, uint32_t pixel, uint32_t frame, int n, float* out) {
  Rekey(seed, pixel, frame, kTagPath);
  for (int i = 0; i < n; i++) out[i] = rt2_ref_uniform();
}

// Closest hit of the scene's top-level list. out: hit, t, point(3), normal(3), front_face, material index,
// uv(2). Media draw from the stream (key, 0xFFFFFFF0, 0), as oracle_scene_hit does.
int ref_hit(void* sp, const float* o, const float* d, float time, float tmin, float tmax, uint64_t key, float* out) {
  const cpu::Scene& s = static_cast<RefScene*>(sp)->scene;
  Rekey(key, 0xFFFFFFF0u, 0, kTagPath);
  const cpu::Ray r{.origin = vec3{o[0], o[1], o[2]}, .direction = vec3{d[0], d[1], d[2]}, .time = time};
  cpu::HitRecord rec{};
  const bool hit = s.hittable_list.Hit(s, r, cpu::Interval{tmin, tmax}, rec);
  out[0] = hit ? 1.f : 0.f;
  out[1] = rec.t;
  out[2] = rec.point.x;
  out[3] = rec.point.y;
  out[4] = rec.point.z;
  out[5] = rec.normal.x;
  out[6] = rec.normal.y;
  out[7] = rec.normal.z;
  out[8] = rec.front_face ? 1.f : 0.f;
  out[9] = hit ? static_cast<float>(rec.material - s.materials.data()) : -1.f;
  out[10] = rec.uv.x;
  out[11] = rec.uv.y;
  return hit ? 1 : 0;
}

// Camera setters (Camera.hpp:69-101): in = center(3) look_at(3) view_up(3) vfov defocus_angle focus_distance
void ref_set_camera(void* sp, const float* in) {
  cpu::Camera& c = static_cast<RefScene*>(sp)->scene.cam;
  c.SetCenter(vec3{in[0], in[1], in[2]});
  c.SetLookAt(vec3{in[3], in[4], in[5]});
  c.SetViewUp(vec3{in[6], in[7], in[8]});
  c.SetFOV(in[9]);
  c.SetDefocusAngle(in[10]);
  c.SetFocusDistance(in[11]);
}

// The 21 words of oracle_camera_params, read from the reference Camera after Update().
int ref_camera(void* sp, int w, int h, int spp, float* out) {
  cpu::Camera c = static_cast<RefScene*>(sp)->scene.cam;
  c.SetDims(glm::ivec2{w, h});
  c.SetSamplesPerPixel(spp);
  c.Update();
  const vec3 v[6] = {c.pixel00_loc_, c.pixel_delta_u_, c.pixel_delta_v_, c.center_, c.defocus_disk_u_, c.defocus_disk_v_};
  for (int i = 0; i < 6; i++) {
    out[3 * i] = v[i].x;
    out[3 * i + 1] = v[i].y;
    out[3 * i + 2] = v[i].z;
  }
  out[18] = c.defocus_angle_;
  out[19] = c.recip_sqrt_samples_per_pix_;
  out[20] = static_cast<float>(c.sqrt_samples_per_pix_);
  return 0;
}

// Frames [frame_begin, frame_begin + frames) of RayTracer::Update at w x h, added to accum (3 floats per
// pixel, row-major). *draws receives the uniforms consumed.
int ref_render(void* sp, int w, int h, int spp, int max_depth, uint64_t seed, int frame_begin, int frames,
               float* accum, uint64_t* draws) {
  const cpu::Scene& s = static_cast<RefScene*>(sp)->scene;
  cpu::Camera cam = s.cam;
  cam.SetSamplesPerPixel(spp);
  cpu::RayTracer rt;
  rt.camera = &cam;
  rt.max_depth = static_cast<size_t>(max_depth);
  rt.OnResize(glm::ivec2{w, h});
  const size_t n = static_cast<size_t>(w) * static_cast<size_t>(h);
  for (size_t i = 0; i < n; i++) rt.accumulation_data_[i] = vec3{accum[3 * i], accum[3 * i + 1], accum[3 * i + 2]};
  uint64_t total = 0;
  for (int y = 0; y < h; y++) {
    for (int x = 0; x < w; x++) {
      const int i = y * w + x;
      for (int f = frame_begin; f < frame_begin + frames; f++) {
        Rekey(seed, static_cast<uint32_t>(i), static_cast<uint32_t>(f), kTagPath);
        rt.iter_.assign(1, glm::ivec3{x, y, i});
        rt.frame_idx_ = static_cast<size_t>(f);
        rt.Update(s);
        total += g_stream.draws;
      }
    }
  }
  for (size_t i = 0; i < n; i++) {
    accum[3 * i] = rt.accumulation_data_[i].x;
    accum[3 * i + 1] = rt.accumulation_data_[i].y;
    accum[3 * i + 2] = rt.accumulation_data_[i].z;
  }
  if (draws) *draws = total;
  return 0;
}

// Noise::Value of texture `tex` at n points (3 floats in, 3 floats out each); -1 if it is no noise texture.
int ref_perlin_probe(void* sp, int tex, const float* points, int n, float* out) {
  const cpu::Scene& s = static_cast<RefScene*>(sp)->scene;
  if (tex < 0 || static_cast<size_t>(tex) >= s.textures.size()) return -1;
  const auto* noise = std::get_if<cpu::texture::Noise>(&s.textures[static_cast<size_t>(tex)]);
  if (!noise) return -1;
  for (int i = 0; i < n; i++) {
    const vec3 v = noise->Value(s.textures, vec2{0, 0}, vec3{points[3 * i], points[3 * i + 1], points[3 * i + 2]});
    out[3 * i] = v.x;
    out[3 * i + 1] = v.y;
    out[3 * i + 2] = v.z;
  }
  return 0;
}

}  // extern "C"
