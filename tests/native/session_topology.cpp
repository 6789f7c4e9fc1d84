// session_topology.cpp -- the host's rule for answering a --start in place (eleven::SessionEdits, elevenrender_amd/host/eleven_host.hpp)
// with the object loads told apart from --load_config, driven without a device: each argument is a session as a string of events --
// s = a --start that succeeds, f = one that fails, c = --load_camera, h = --load_hdri, m = --load_brdf_material or --load_texture,
// o = --load_object, g = --load_config -- and for each the program prints, per --start, c if it would take the in-place camera update,
// e if the in-place scene edit, t if the in-place topology edit and 0 if the full start_rendering.  At most one of the three
// predicates may hold; two at once print '!'.  (tests/test_topology_cpu.py)
#include <cstdio>

#include "../../elevenrender_amd/host/eleven_host.hpp"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        eleven::SessionEdits e;
        for (const char* p = argv[a]; *p; p++) {
            if (*p == 'c') e.on_camera();
            else if (*p == 'h') e.on_hdri();
            else if (*p == 'm') e.on_materials();
            else if (*p == 'o') e.on_object();
            else if (*p == 'g') e.on_other();
            else if (*p == 's' || *p == 'f') {
                const int n = (e.camera_only() ? 1 : 0) + (e.editable() ? 1 : 0) + (e.appendable() ? 1 : 0);
                std::putchar(n > 1 ? '!' : e.camera_only() ? 'c' : e.editable() ? 'e' : e.appendable() ? 't' : '0');
                if (*p == 's') e.on_started();
                else e.on_failed();
            }
        }
        std::putchar('\n');
    }
    return 0;
}
