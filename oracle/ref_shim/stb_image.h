// Stand-in for stb_image.h, written from the public stb_image API names only (oracle/ref_shim/README.md): the five entry points the
// reference's texture loader names, loading nothing -- the fixtures hand texel arrays over, never files.
#pragma once
#include <iostream>
inline void stbi_ldr_to_hdr_gamma(float) {}
inline void stbi_set_flip_vertically_on_load(int) {}
inline float* stbi_loadf(const char*, int* x, int* y, int* channels_in_file, int) {
    *x = *y = *channels_in_file = 0;
    return nullptr;
}
inline void stbi_image_free(void*) {}
inline const char* stbi_failure_reason() { return "stand-in: no image loading"; }
