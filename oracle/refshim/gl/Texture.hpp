// Stub of the reference's gl/Texture.hpp for the reference build: RayTracer holds one by value and the
// CPU render path never touches it.
#pragma once
namespace gl {
class Texture {};
}  // namespace gl
