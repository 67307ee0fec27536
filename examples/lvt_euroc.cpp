// lvt_euroc -- EuRoC MAV stereo command line harness over the C-ABI (SURVEY 8(f) rows 1 + 2).
//
// Same argv, inputs and outputs as the reference's example binary (examples/euroc/euroc_example.cpp:49-175 there):
//     lvt_euroc <euroc_root_dir> <stamps_dir> <dataset_name> <config_file_name> [--max-frames N] [--out name.txt] [--clahe CLIP[,TX,TY]] [--lens FILE] [--mono16 LO,HI|auto[,LOPM,HIPM,SPAN]]
// (--clahe: CLAHE contrast equalisation of the rectified frames inside the feature stage, lvt_amd_set_equalisation; absent by default)
// reads <stamps_dir>/<dataset_name>.txt (one nanosecond stamp per line = the image file stem), the cam0 / cam1 PNGs below
// <root>/<dataset_name>/mav0/, hands the RAW images to lvt_track -- the two rectifiers with the calibration the reference hard-codes
// (lvt_amd_rectifier_*: cv::initUndistortRectifyMap + cv::remap INTER_LINEAR) are attached to the tracker once, which rectifies
// every frame at the head of its feature stage (lvt_amd_set_rectifiers) --, maps the camera pose into the body
// frame (T_BS * T_cam) and writes <dataset_name>.txt in the TUM format "t x y z qx qy qz qw" (6 / 7 digits).
//
// --lens FILE (not in the reference): the calibration comes from FILE instead of the hard-coded EuRoC one, so any folder of the same mav0 layout runs -- a
// TUM-VI sequence with its equidistant lenses, a rational-polynomial rig, raw images of another size than the tracked one ("LENS MODELS",
// include/lvt_amd_ext.h).  FILE is flat `key: number` lines (what the config reader takes; # starts a comment, a missing key reads as 0):
//     dst_width, dst_height      the rectified (tracked) size
//     P0 ... P8                  the new camera matrix, row-major; fx fy cx cy of the tracker are P0 P4 P2 P5
//     baseline                   metres
//     left_model, right_model    0 = radtan (plumb_bob / rational_polynomial), 1 = fisheye (equidistant)
//     left_width, left_height    the RAW image's size (right_ likewise; the two are equal)
//     left_K0 ... left_K8        the raw camera matrix, row-major;  left_D0 ... left_D11  the coefficients;  left_R0 ... left_R8  the rectifying rotation
//     Tbs0 ... Tbs11             (optional) body-from-camera, 3 x 4 row-major; absent: the identity, the trajectory is the left camera's
//
// --mono16 LO,HI | auto[,LOPM,HIPM,SPAN] (not in the reference): the images are 16-bit binary PGMs (<stamp>.pgm, maxval > 255: thermal cameras, 10 / 12-bit
// machine vision) and go to the tracker as they are, LVT_AMD_SENSOR_MONO16 ("SENSOR FORMATS", include/lvt_amd_ext.h): a fixed window [LO, HI], or one found per
// frame from the frame's histogram with LOPM / HIPM permille of the pixels allowed below / above it and a smallest width SPAN (defaults 5, 5, 256).
#include "../include/lvt_amd_ext.h"
#include "../include/lvt_c.h"
#include "image_io.h"

#include <chrono>
#include <cstdio>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <utility>

using namespace lvt_io;

namespace {

// Eigen::Quaternion(Matrix3) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other,3,3>): w x y z
void rotation_to_quaternion(const double m[3][3], double q[4]) {
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m[2][1] - m[1][2]) * t;
        q[2] = (m[0][2] - m[2][0]) * t;
        q[3] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[k][j] - m[j][k]) * t;
        q[1 + j] = (m[j][i] + m[i][j]) * t;
        q[1 + k] = (m[k][i] + m[i][k]) * t;
    }
}

// the flat `key: number` reader of the config files (lvt_amd_params_from_file's rules): # starts a comment, a line without a number behind its colon is skipped
bool read_numbers(const std::string &path, std::vector<std::pair<std::string, double>> &kv) {
    std::ifstream f(path);
    if (!f.is_open()) return false;
    std::string line;
    while (std::getline(f, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.erase(hash);
        const size_t colon = line.find(':');
        if (colon == std::string::npos || line[0] == '%') continue;
        const size_t a = line.find_first_not_of(" \t"), b = line.find_last_not_of(" \t", colon ? colon - 1 : 0);
        if (a == std::string::npos || a >= colon) continue;
        const char *num = line.c_str() + colon + 1;
        char *end = nullptr;
        const double v = std::strtod(num, &end);
        if (end == num) continue;
        kv.emplace_back(line.substr(a, b - a + 1), v);
    }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 5) {
        std::cout << "Usage ./lvt_euroc euroc_root_dir stamps_dir dataset_name config_file_name [--max-frames N] [--out name.txt] [--clahe CLIP[,TX,TY]] [--lens FILE] [--mono16 LO,HI|auto[,LOPM,HIPM,SPAN]]" << std::endl;
        return -1;
    }
    const std::string root_dir = argv[1], stamps_dir = argv[2], dataset_name = argv[3], config_file_name = argv[4];
    const std::string seq_dir = root_dir + "/" + dataset_name + "/mav0";
    std::string out_name = dataset_name + ".txt";
    long max_frames = -1;
    std::string lens_file;  // --lens FILE: the calibration of both eyes, P and the tracked size
    lvt_amd_equalisation clahe = {0, 0, 0.f};  // --clahe CLIP[,TX,TY]: equalise the rectified frames (dark sequences); tiles 8 x 8 unless given
    lvt_amd_sensor_format mono16 = {LVT_AMD_SENSOR_NONE, 0, 0, 0, 5, 5, 256, {0}};  // --mono16: 16-bit PGMs, mapped to 8 bits inside the feature stage
    for (int i = 5; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--mono16") {
            const std::string v = argv[i + 1];
            mono16.format = LVT_AMD_SENSOR_MONO16;
            if (v.compare(0, 4, "auto") == 0) {
                mono16.auto_window = 1;
                if (v.size() > 4 && std::sscanf(v.c_str() + 4, ",%d,%d,%d", &mono16.lo_permille, &mono16.hi_permille, &mono16.min_span) < 1) mono16.format = -1;
            } else if (std::sscanf(v.c_str(), "%d,%d", &mono16.lo, &mono16.hi) != 2) {
                mono16.format = -1;
            }
            if (mono16.format < 0) {
                std::cout << "--mono16 LO,HI|auto[,LOPM,HIPM,SPAN]: cannot read " << v << std::endl;
                return -1;
            }
        } else if (k == "--out") out_name = argv[i + 1];
        else if (k == "--max-frames") max_frames = std::atol(argv[i + 1]);
        else if (k == "--lens") lens_file = argv[i + 1];
        else if (k == "--clahe") {
            clahe.tiles_x = clahe.tiles_y = 8;
            if (std::sscanf(argv[i + 1], "%f,%d,%d", &clahe.clip_limit, &clahe.tiles_x, &clahe.tiles_y) < 1) {
                std::cout << "--clahe CLIP[,TX,TY]: cannot read " << argv[i + 1] << std::endl;
                return -1;
            }
        }
    }
    std::vector<std::string> titles;
    std::vector<double> time_stamps;
    {
        const std::string path = stamps_dir + "/" + dataset_name + ".txt";
        std::ifstream f(path);
        if (!f.is_open()) {
            std::cout << "Unable to open stamps files " << path << std::endl;
            return -1;
        }
        std::string line;
        while (std::getline(f, line)) {
            while (!line.empty() && std::isspace((unsigned char)line.back())) line.pop_back();
            if (line.empty()) continue;
            titles.push_back(line + (mono16.format ? ".pgm" : ".png"));
            time_stamps.push_back(std::atof(line.c_str()) / 1e9);
        }
    }
    lvt_amd_params params;
    if (!lvt_amd_params_from_file(config_file_name.c_str(), &params)) {
        std::cout << "Failed to initialize from " << config_file_name << std::endl;
        return -1;
    }
    // the calibration of the reference's example (euroc_example.cpp:95-119)
    const double kl[9] = {458.654, 0.0, 367.215, 0.0, 457.296, 248.375, 0.0, 0.0, 1.0};
    const double kr[9] = {457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1.0};
    const double pn[9] = {435.2046959714599, 0, 367.4517211914062, 0, 435.2046959714599, 252.2008514404297, 0, 0, 1};
    const double rl[9] = {0.999966347530033, -0.001422739138722922, 0.008079580483432283, 0.001365741834644127, 0.9999741760894847,
                          0.007055629199258132, -0.008089410156878961, -0.007044357138835809, 0.9999424675829176};
    const double rr[9] = {0.9999633526194376, -0.003625811871560086, 0.007755443660172947, 0.003680398547259526, 0.9999684752771629,
                          -0.007035845251224894, -0.007729688520722713, 0.007064130529506649, 0.999945173484644};
    const double dl[5] = {-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0};
    const double dr[5] = {-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0};
    int W = 752, H = 480;    // the RAW images' size
    params.fx = 435.2046959714599f, params.fy = 435.2046959714599f, params.cx = 367.4517211914062f, params.cy = 252.2008514404297f;
    params.baseline = 0.110077842f;
    params.img_width = W, params.img_height = H;
    double Tbs[4][4] = {{0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975},
                              {0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768},
                              {-0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949},
                              {0.0, 0.0, 0.0, 1.0}};
    lvt_amd_rectifier rect_l = nullptr, rect_r = nullptr;
    if (lens_file.empty()) {
        rect_l = lvt_amd_rectifier_create(kl, dl, rl, pn, W, H), rect_r = lvt_amd_rectifier_create(kr, dr, rr, pn, W, H);
    } else {
        std::vector<std::pair<std::string, double>> kv;
        if (!read_numbers(lens_file, kv)) {
            std::cout << "Unable to open the lens file " << lens_file << std::endl;
            return -1;
        }
        bool has_tbs = false;
        auto get = [&](const std::string &k) -> double {
            for (auto &e : kv)
                if (e.first == k) return e.second;
            return 0.0;
        };
        for (auto &e : kv) has_tbs = has_tbs || e.first.compare(0, 3, "Tbs") == 0;
        double P[9];
        for (int k = 0; k < 9; k++) P[k] = get("P" + std::to_string(k));
        const int dw = (int)std::nearbyint(get("dst_width")), dh = (int)std::nearbyint(get("dst_height"));
        lvt_amd_lens lens[2];
        double Rr[2][9];
        for (int e = 0; e < 2; e++) {
            const std::string eye = e ? "right_" : "left_";
            lens[e].model = (int)std::nearbyint(get(eye + "model"));
            lens[e].width = (int)std::nearbyint(get(eye + "width")), lens[e].height = (int)std::nearbyint(get(eye + "height"));
            for (int k = 0; k < 9; k++) lens[e].K[k] = get(eye + "K" + std::to_string(k)), Rr[e][k] = get(eye + "R" + std::to_string(k));
            for (int k = 0; k < 12; k++) lens[e].D[k] = get(eye + "D" + std::to_string(k));
        }
        params.fx = (float)P[0], params.fy = (float)P[4], params.cx = (float)P[2], params.cy = (float)P[5];
        params.baseline = (float)get("baseline");
        params.img_width = dw, params.img_height = dh;
        W = lens[0].width, H = lens[0].height;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) Tbs[r][c] = has_tbs ? get("Tbs" + std::to_string(4 * r + c)) : (r == c ? 1.0 : 0.0);
        rect_l = lvt_amd_rectifier_create_lens(&lens[0], Rr[0], P, dw, dh);
        if (rect_l) rect_r = lvt_amd_rectifier_create_lens(&lens[1], Rr[1], P, dw, dh);
    }
    lvt_handle vo = lvt_amd_create(&params, 1 /* STEREO */);
    if (!rect_l || !rect_r || !vo) {
        std::cout << "failed to create the tracker: " << lvt_amd_last_error(nullptr) << std::endl;
        return -1;
    }
    if (lvt_amd_set_rectifiers(vo, rect_l, rect_r) != 0) {  // from here on lvt_track takes the camera's raw images
        std::cout << "failed to attach the rectifiers: " << lvt_amd_last_error(vo) << std::endl;
        return -1;
    }
    if (clahe.tiles_x && lvt_amd_set_equalisation(vo, &clahe) != 0) {
        std::cout << "failed to set the equalisation: " << lvt_amd_last_error(vo) << std::endl;
        return -1;
    }
    if (mono16.format && lvt_amd_set_sensor_format(vo, &mono16) != 0) {
        std::cout << "failed to set the sensor format: " << lvt_amd_last_error(vo) << std::endl;
        return -1;
    }
    long frame_count = (long)titles.size();
    if (max_frames >= 0 && max_frames < frame_count) frame_count = max_frames;
    std::vector<double> poses;  // q (w x y z), p of the BODY per processed frame
    double total_time = 0;
    long n = 0;
    for (long i = 0; i < frame_count; i++) {
        std::cout << "Frame number: " << i << "/" << frame_count << "\r" << std::flush;
        Gray left, right;
        std::string err;
        if (!load_image(seq_dir + "/cam0/data/" + titles[i], left, err) || !load_image(seq_dir + "/cam1/data/" + titles[i], right, err) || left.w != W ||
            left.h != H || right.w != W || right.h != H || (mono16.format && (left.px16.empty() || right.px16.empty()))) {
            std::cout << "Failed to load image " << titles[i] << (mono16.format ? " (--mono16 takes binary PGMs with maxval > 255)" : "") << std::endl;
            break;
        }
        const auto t0 = std::chrono::steady_clock::now();
        double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
        if (mono16.format) lvt_track(vo, reinterpret_cast<unsigned char *>(left.px16.data()), reinterpret_cast<unsigned char *>(right.px16.data()), H, W, R, t);
        else lvt_track(vo, left.px.data(), right.px.data(), H, W, R, t);
        total_time += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        double body[3][4];  // Tbs * [R t; 0 1]
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) {
                double s = 0;
                for (int k = 0; k < 3; k++) s += Tbs[r][k] * (c < 3 ? R[k][c] : t[k]);
                body[r][c] = s + (c == 3 ? Tbs[r][3] : 0.0);
            }
        const double Rb[3][3] = {{body[0][0], body[0][1], body[0][2]}, {body[1][0], body[1][1], body[1][2]}, {body[2][0], body[2][1], body[2][2]}};
        double q[4];
        rotation_to_quaternion(Rb, q);
        for (int k = 0; k < 4; k++) poses.push_back(q[k]);
        for (int k = 0; k < 3; k++) poses.push_back(body[k][3]);
        n++;
        if (lvt_get_status(vo) == 3) break;  // LOST
    }
    std::ofstream file(out_name.c_str());
    file << std::fixed;
    for (long i = 0; i < (long)titles.size(); i++) {
        double q[4] = {1, 0, 0, 0}, p[3] = {0, 0, 0};
        if (i < n) {
            for (int k = 0; k < 4; k++) q[k] = poses[(size_t)i * 7 + k];
            for (int k = 0; k < 3; k++) p[k] = poses[(size_t)i * 7 + 4 + k];
        }
        file << std::setprecision(6) << time_stamps[i] << std::setprecision(7) << " " << p[0] << " " << p[1] << " " << p[2] << " " << q[1] << " " << q[2]
             << " " << q[3] << " " << q[0] << std::endl;
    }
    file.close();
    lvt_destroy(vo);
    lvt_amd_rectifier_destroy(rect_l);
    lvt_amd_rectifier_destroy(rect_r);
    std::cout << std::endl << "Frames: " << n << "/" << frame_count << "  Average frame processing time (rectify + track): " << (n ? total_time / (double)n : 0.0) << std::endl;
    return 0;
}
