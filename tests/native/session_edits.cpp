// session_edits.cpp -- the host's rule for restarting a render in place (eleven::SessionEdits, elevenrender_amd/host/eleven_host.hpp),
// driven without a device: each argument is a session as a string of events -- s = a --start that succeeds, f = a --start that
// fails, c = --load_camera, o = any other load -- and for each the program prints, per --start, 1 if it would take the in-place
// camera update and 0 if the full start_rendering.  (tests/test_update_cpu.py)
#include <cstdio>

#include "../../elevenrender_amd/host/eleven_host.hpp"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        eleven::SessionEdits e;
        for (const char* p = argv[a]; *p; p++) {
            if (*p == 'c') e.on_camera();
            else if (*p == 'o') e.on_other();
            else if (*p == 's' || *p == 'f') {
                std::putchar(e.camera_only() ? '1' : '0');
                if (*p == 's') e.on_started();
                else e.on_failed();
            }
        }
        std::putchar('\n');
    }
    return 0;
}
