// Prints what tools/camera_info_yaml.hpp reads from each file given (tests/test_camera_info_yaml.py): one line per file,
// "width height n_d K[9] D[n_d] R[9] P[12]" with 17 significant digits, or "ERROR <message>".
#include <cstdio>
#include "camera_info_yaml.hpp"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        svo_camera_info ci; std::string err;
        if (!camera_info_yaml::load(argv[a], ci, err)) { std::printf("ERROR %s\n", err.c_str()); continue; }
        std::printf("%d %d %d", ci.width, ci.height, ci.n_d);
        for (double v : ci.K) std::printf(" %.17g", v);
        for (int i = 0; i < ci.n_d; i++) std::printf(" %.17g", ci.D[i]);
        for (double v : ci.R) std::printf(" %.17g", v);
        for (double v : ci.P) std::printf(" %.17g", v);
        std::printf("\n");
    }
    return 0;
}
