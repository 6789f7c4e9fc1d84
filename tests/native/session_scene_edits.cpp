// session_scene_edits.cpp -- the host's rule for answering a --start in place (eleven::SessionEdits, elevenrender_amd/host/eleven_host.hpp)
// with the material, texture and HDRI loads told apart, driven without a device: each argument is a session as a string of events --
// s = a --start that succeeds, f = one that fails, c = --load_camera, h = --load_hdri, m = --load_brdf_material or --load_texture,
// o = --load_object or --load_config -- and for each the program prints, per --start, c if it would take the in-place camera update,
// e if the in-place scene edit and 0 if the full start_rendering.  (tests/test_edit_cpu.py)
#include <cstdio>

#include "../../elevenrender_amd/host/eleven_host.hpp"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        eleven::SessionEdits e;
        for (const char* p = argv[a]; *p; p++) {
            if (*p == 'c') e.on_camera();
            else if (*p == 'h') e.on_hdri();
            else if (*p == 'm') e.on_materials();
            else if (*p == 'o') e.on_other();
            else if (*p == 's' || *p == 'f') {
                std::putchar(e.camera_only() ? 'c' : (e.editable() ? 'e' : '0'));
                if (*p == 's') e.on_started();
                else e.on_failed();
            }
        }
        std::putchar('\n');
    }
    return 0;
}
