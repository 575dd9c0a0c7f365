// camera_info_yaml.hpp — reads a ROS camera_calibration_parsers YAML file (what camera_calibration writes and
// camera_info_manager loads: image_width, image_height, camera_matrix, distortion_model, distortion_coefficients,
// rectification_matrix, projection_matrix; matrices as {rows, cols, data: [...]}) into an svo_camera_info.  Header-only, no
// YAML library: the format is flat and written by one tool, so a key scan and a flow-sequence number reader suffice.
// Distortion models: plumb_bob (5 coefficients; 4 accepted) and rational_polynomial (8); others (equidistant / fisheye) are
// refused — the library's generator does not cover them.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "svo.h"

namespace camera_info_yaml {

// position just after "key:" at the start of a line (leading spaces allowed), or npos
inline size_t find_key(const std::string& t, const std::string& key, size_t from = 0) {
    for (size_t p = t.find(key + ":", from); p != std::string::npos; p = t.find(key + ":", p + 1)) {
        size_t b = p;
        while (b > 0 && (t[b - 1] == ' ' || t[b - 1] == '\t')) b--;
        if (b == 0 || t[b - 1] == '\n') return p + key.size() + 1;
    }
    return std::string::npos;
}
inline std::string scalar(const std::string& t, const std::string& key) {
    size_t p = find_key(t, key);
    if (p == std::string::npos) return "";
    size_t e = t.find('\n', p);
    std::string v = t.substr(p, e == std::string::npos ? std::string::npos : e - p);
    const size_t a = v.find_first_not_of(" \t\"'"), z = v.find_last_not_of(" \t\r\"'");
    return a == std::string::npos ? "" : v.substr(a, z - a + 1);
}
// the numbers of `key: {rows, cols, data: [...]}` (block or flow mapping; data may span lines)
inline bool matrix(const std::string& t, const std::string& key, std::vector<double>& out, int* rows = nullptr, int* cols = nullptr) {
    size_t p = find_key(t, key);
    if (p == std::string::npos) return false;
    size_t next = t.find('\n', p);                                  // the matrix ends at the next top-level key
    while (next != std::string::npos && next + 1 < t.size() && (t[next + 1] == ' ' || t[next + 1] == '\t' || t[next + 1] == '\n')) next = t.find('\n', next + 1);
    const std::string body = t.substr(p, next == std::string::npos ? std::string::npos : next - p);
    auto num_after = [&](const char* k) { size_t q = body.find(k); return q == std::string::npos ? -1 : std::atoi(body.c_str() + q + std::strlen(k)); };
    if (rows) *rows = num_after("rows:");
    if (cols) *cols = num_after("cols:");
    size_t d = body.find("data:");
    if (d == std::string::npos) return false;
    size_t a = body.find('[', d), z = body.find(']', d);
    if (a == std::string::npos || z == std::string::npos || z < a) return false;
    std::string s = body.substr(a + 1, z - a - 1);
    for (char& c : s) if (c == ',' || c == '\n' || c == '\r' || c == '\t') c = ' ';
    out.clear();
    std::istringstream in(s);
    std::string tok;
    while (in >> tok) {
        char* end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str()) return false;
        out.push_back(v);
    }
    return true;
}

// Fills ci; on failure returns false and sets err.
inline bool parse(const std::string& text, svo_camera_info& ci, std::string& err) {
    std::string t;                                                  // comments stripped
    {
        std::istringstream in(text);
        std::string line;
        while (std::getline(in, line)) { const size_t h = line.find('#'); t += (h == std::string::npos ? line : line.substr(0, h)) + "\n"; }
    }
    ci = svo_camera_info{};
    const std::string w = scalar(t, "image_width"), h = scalar(t, "image_height");
    if (w.empty() || h.empty()) { err = "image_width / image_height missing"; return false; }
    ci.width = std::atoi(w.c_str()); ci.height = std::atoi(h.c_str());
    std::vector<double> K, D, R, P;
    if (!matrix(t, "camera_matrix", K) || K.size() != 9) { err = "camera_matrix must hold 9 numbers"; return false; }
    if (!matrix(t, "projection_matrix", P) || P.size() != 12) { err = "projection_matrix must hold 12 numbers"; return false; }
    if (!matrix(t, "rectification_matrix", R)) R = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (R.size() != 9) { err = "rectification_matrix must hold 9 numbers"; return false; }
    if (!matrix(t, "distortion_coefficients", D)) D.clear();
    std::string model = scalar(t, "distortion_model");
    if (model.empty()) model = "plumb_bob";
    if (model == "plumb_bob" ? !(D.size() == 5 || D.size() == 4 || D.empty()) : model == "rational_polynomial" ? D.size() != 8 : true) {
        err = "distortion_model " + model + " with " + std::to_string(D.size()) + " coefficients is not supported (plumb_bob 5, rational_polynomial 8)";
        return false;
    }
    for (int i = 0; i < 9; i++) { ci.K[i] = K[i]; ci.R[i] = R[i]; }
    for (int i = 0; i < 12; i++) ci.P[i] = P[i];
    ci.n_d = (int)D.size();
    for (int i = 0; i < ci.n_d; i++) ci.D[i] = D[i];
    return true;
}
inline bool load(const std::string& path, svo_camera_info& ci, std::string& err) {
    std::ifstream f(path);
    if (!f) { err = "cannot open " + path; return false; }
    std::stringstream ss; ss << f.rdbuf();
    return parse(ss.str(), ci, err);
}

}   // namespace camera_info_yaml
