// lvt_kitti -- KITTI-odometry command line harness, written against the header-compatible C++ layer
// include/lvt_system.h -- the calls below are the reference example's own (kitti_example.cpp:82-131: lvt_parameters,
// lvt_system::create, vo->track, lvt_pose::get_position / get_orientation_matrix), with lvt_image_view where it has cv::Mat.
//
// Same argv, inputs and outputs as the reference's example binary (examples/kitti/kitti_example.cpp:49-152 there):
//     lvt_kitti <sequences_dir> <seq_number> [--config vo_config.yaml] [--calib calib/NN.yml] [--max-frames N] [--out NN.txt] [--covariance FILE]
//                [--mask LEFT[,RIGHT]] [--labels DIR --drop L1,L2,... [--dilate R]]
// reads <sequences_dir>/NN/image_0/%06d.{png,pgm} and image_1/..., the OpenCV-YAML calibration (camera_matrix, baseline)
// and vo_config.yaml, tracks every frame until the sequence ends or the tracker is LOST, writes NN.txt in the KITTI
// 3x4 row format with the reference's precision (fixed, 9 digits) and prints the mean per-frame track() time.
// No OpenCV: the PNG reader below handles what KITTI ships (8-bit gray / RGB / RGBA / gray+alpha, non-interlaced), colour
// is reduced to gray with cv::cvtColor's fixed-point weights, and PGM (P5) is accepted for pre-converted data.
// --covariance FILE (not in the reference): the tracker also evaluates every frame's pose uncertainty (lvt_system::enable_pose_info) and FILE receives one
// line per tracked frame: frame, status, n_inliers and the six sigmas (square roots of the covariance's diagonal: metres x y z, radians x y z; zeros
// unless the status is 1).  Without the option nothing of this runs.
// --mask LEFT[,RIGHT] (not in the reference): feature masks (lvt_system::set_mask), 8-bit PNG or PGM files of the frames' size, a pixel != 0: key points
// allowed -- the ego vehicle's bonnet, an overlay.  LEFT alone masks the left eye only.  A file of another size is refused before the first frame.
// --labels DIR --drop L1,L2,... [--dilate R] (not in the reference): per-frame label masks (lvt_system::set_label_mask / frame_labels).  DIR/%06d.png
// (or .pgm), an 8-bit image of ANY size -- a segmentation network's output, usually a fraction of the frame's -- holds the left eye's labels of that frame;
// key points on pixels whose label is among L1,L2,..., widened by R pixels (0 ... 15, default 0), are dropped.  The first file fixes the label size; a frame
// whose file is missing gets no labels.  The same trajectory format.
// --bayer RGGB|BGGR|GRBG|GBRG (not in the reference): the files are 8-bit Bayer mosaics as a machine-vision camera delivers them (8-bit gray PNG or PGM whose
// pixels are the samples); they go to the tracker as they are and are demosaiced to gray inside the feature stage (lvt_system::set_sensor_format, "SENSOR
// FORMATS" in include/lvt_amd_ext.h).
#include "../include/lvt_system.h"

#include "image_io.h"

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace lvt_io;

namespace {

// the two entries the reference reads from calib/NN.yml (OpenCV FileStorage YAML): camera_matrix.data and baseline
bool read_calib(const std::string &path, double K[9], double &baseline) {
    std::ifstream f(path);
    if (!f) return false;
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string s = ss.str();
    const size_t cm = s.find("camera_matrix");
    const size_t d0 = (cm == std::string::npos) ? cm : s.find("data:", cm);
    const size_t b0 = s.find("baseline:");
    if (d0 == std::string::npos || b0 == std::string::npos) return false;
    const size_t lb = s.find('[', d0), rb = s.find(']', d0);
    if (lb == std::string::npos || rb == std::string::npos) return false;
    std::string list = s.substr(lb + 1, rb - lb - 1);
    for (char &c : list)
        if (c == ',') c = ' ';
    std::stringstream ls(list);
    for (int i = 0; i < 9; i++)
        if (!(ls >> K[i])) return false;
    baseline = std::atof(s.c_str() + b0 + 9);
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        std::cout << "Usage ./lvt_kitti sequences_dir seq_number [--config vo_config.yaml] [--calib calib/NN.yml] [--max-frames N] [--out NN.txt] [--reduce F] [--bayer RGGB|BGGR|GRBG|GBRG]" << std::endl;
        return -1;
    }
    char seq_cstr[16];
    std::snprintf(seq_cstr, sizeof seq_cstr, "%02d", std::atoi(argv[2]));
    const std::string seq_str(seq_cstr), dir_prefix = std::string(argv[1]) + "/" + seq_str;
    std::string config = "vo_config.yaml", calib = "calib/" + seq_str + ".yml", out_name = seq_str + ".txt", cov_name, mask_names, labels_dir, drop_list;
    int dilate = 0, reduce = 1;
    std::string bayer;  // --bayer PATTERN: the files are 8-bit Bayer mosaics, demosaiced to gray inside the feature stage (lvt_system::set_sensor_format)
    long max_frames = -1;
    for (int i = 3; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--config") config = argv[i + 1];
        else if (k == "--calib") calib = argv[i + 1];
        else if (k == "--out") out_name = argv[i + 1];
        else if (k == "--max-frames") max_frames = std::atol(argv[i + 1]);
        else if (k == "--covariance") cov_name = argv[i + 1];
        else if (k == "--mask") mask_names = argv[i + 1];
        else if (k == "--labels") labels_dir = argv[i + 1];
        else if (k == "--drop") drop_list = argv[i + 1];
        else if (k == "--dilate") dilate = std::atoi(argv[i + 1]);
        else if (k == "--reduce") reduce = std::atoi(argv[i + 1]);
        else if (k == "--bayer") bayer = argv[i + 1];
    }
    double K[9], baseline = 0;
    if (!read_calib(calib, K, baseline)) {
        std::cout << "failed to open camera matrix yml file" << std::endl;
        return -1;
    }
    lvt_parameters params;
    if (!params.init_from_file(config.c_str())) {
        std::cout << "failed to initialize from vo_config.yml file." << std::endl;
        return -1;
    }
    auto stem = [&](int cam, long i) {
        char name[32];
        std::snprintf(name, sizeof name, "/image_%d/%06ld", cam, i);
        return dir_prefix + name;
    };
    Gray left, right;
    std::string err;
    if (!load_gray(stem(0, 0), left, err) || !load_gray(stem(1, 0), right, err)) {
        std::cout << "failed to get image sequences (" << err << ")" << std::endl;
        return -1;
    }
    // --reduce F: the PNGs are F times the size the tracker runs at.  The tracker is created at W / F x H / F with the calibration of the REDUCED image (reduced
    // pixel x covers source columns [F x, F x + F): f' = f / F, c' = (c + 0.5) / F - 0.5, in double) and is handed the decoded full-size frames.
    if (reduce < 1 || reduce > 8 || left.w / reduce < 1 || left.h / reduce < 1) {
        std::cout << "--reduce takes a factor 1 ... 8 that leaves at least one pixel each way" << std::endl;
        return -1;
    }
    const int frame_w = left.w, frame_h = left.h;
    const double F = (double)reduce;
    if (reduce > 1) K[0] /= F, K[4] /= F, K[2] = (K[2] + 0.5) / F - 0.5, K[5] = (K[5] + 0.5) / F - 0.5;
    params.fx = (float)K[0], params.fy = (float)K[4], params.cx = (float)K[2], params.cy = (float)K[5];
    params.baseline = (float)baseline;
    params.img_width = frame_w / reduce, params.img_height = frame_h / reduce;
    lvt_system *vo = lvt_system::create(params, lvt_system::eSensor_STEREO);
    if (!vo) {
        std::cout << "failed to create the tracker: " << lvt_amd_last_error(nullptr) << std::endl;
        return -1;
    }
    if (!bayer.empty()) {
        lvt_amd_sensor_format sf = {LVT_AMD_SENSOR_NONE, 0, 0, 0, 0, 0, 0, {0}};
        sf.format = bayer == "RGGB" ? LVT_AMD_SENSOR_BAYER_RGGB8 : bayer == "BGGR" ? LVT_AMD_SENSOR_BAYER_BGGR8 : bayer == "GRBG" ? LVT_AMD_SENSOR_BAYER_GRBG8 : bayer == "GBRG" ? LVT_AMD_SENSOR_BAYER_GBRG8 : -1;
        if (sf.format < 0) {
            std::cout << "--bayer takes RGGB, BGGR, GRBG or GBRG" << std::endl;
            lvt_system::destroy(vo);
            return -1;
        }
        if (!vo->set_sensor_format(&sf)) {
            std::cout << "failed to set the sensor format: " << vo->last_error() << std::endl;
            lvt_system::destroy(vo);
            return -1;
        }
    }
    if (reduce > 1 && !vo->set_reduction(reduce, frame_w, frame_h)) {
        std::cout << "failed to set the reduction: " << vo->last_error() << std::endl;
        lvt_system::destroy(vo);
        return -1;
    }
    std::ofstream cov_file;
    if (!cov_name.empty()) {
        cov_file.open(cov_name.c_str());
        if (!cov_file || !vo->enable_pose_info()) {
            std::cout << "failed to set up the covariance output: " << (cov_file ? vo->last_error() : "cannot open the file") << std::endl;
            lvt_system::destroy(vo);
            return -1;
        }
        cov_file << std::scientific << std::setprecision(9);
    }
    if (!mask_names.empty()) {
        const size_t comma = mask_names.find(',');
        const std::string names[2] = {mask_names.substr(0, comma), comma == std::string::npos ? std::string() : mask_names.substr(comma + 1)};
        Gray mask[2];
        for (int e = 0; e < 2; e++) {
            if (names[e].empty()) continue;
            if (!load_image(names[e], mask[e], err)) {
                std::cout << "failed to read the mask " << names[e] << " (" << err << ")" << std::endl;
                lvt_system::destroy(vo);
                return -1;
            }
            if (mask[e].w != params.img_width || mask[e].h != params.img_height) {  // (the detector's grid: with --reduce the reduced image's)
                std::cout << "the mask " << names[e] << " is " << mask[e].w << " x " << mask[e].h << ", the frames are " << params.img_width << " x " << params.img_height
                          << (reduce > 1 ? " behind the reduction" : "") << std::endl;
                lvt_system::destroy(vo);
                return -1;
            }
        }
        if (!vo->set_mask(names[0].empty() ? nullptr : mask[0].px.data(), names[1].empty() ? nullptr : mask[1].px.data())) {
            std::cout << "failed to set the mask: " << vo->last_error() << std::endl;
            lvt_system::destroy(vo);
            return -1;
        }
    }
    auto label_name = [&](long i) {
        char name[32];
        std::snprintf(name, sizeof name, "/%06ld.png", i);
        return labels_dir + name;
    };
    Gray labels;
    lvt_amd_label_mask label_cfg{};
    if (!labels_dir.empty()) {
        if (!load_image(label_name(0), labels, err)) {
            std::cout << "failed to read the labels " << label_name(0) << " (" << err << ")" << std::endl;
            lvt_system::destroy(vo);
            return -1;
        }
        label_cfg.label_width = labels.w, label_cfg.label_height = labels.h, label_cfg.dilate = dilate;
        std::stringstream ds(drop_list);
        for (std::string item; std::getline(ds, item, ',');) {
            const int l = std::atoi(item.c_str());
            if (item.empty() || l < 0 || l > 255) {
                std::cout << "--drop takes labels 0 ... 255, separated by commas" << std::endl;
                lvt_system::destroy(vo);
                return -1;
            }
            label_cfg.drop[l] = 1;
        }
        if (!vo->set_label_mask(&label_cfg)) {
            std::cout << "failed to set the label mask: " << vo->last_error() << std::endl;
            lvt_system::destroy(vo);
            return -1;
        }
    }
    // like the reference, the trajectory has one row per frame of the sequence; frames after a LOST keep the default pose
    long frame_count = 0;
    for (;; frame_count++) {
        std::ifstream pl(stem(0, frame_count) + ".png"), gl(stem(0, frame_count) + ".pgm");
        if (!pl && !gl) break;
        if (max_frames >= 0 && frame_count >= max_frames) break;
    }
    std::vector<double> rows;  // 12 per processed frame
    double total_time = 0.0;
    long n = 0;
    // Frame i is enqueued (lvt_system::track_async: its images are the library's when the call returns), frame i + 1 is read and decoded while it
    // tracks, then frame i's pose is collected: the reference's loop (kitti_example.cpp:113-138) does the two in turn.  Same poses, same file.
    Gray nleft, nright;
    bool have = true;
    for (long i = 0; i < frame_count && have; i++) {
        if (left.w != frame_w || left.h != frame_h || right.w != left.w || right.h != left.h) {
            std::cout << "frame " << i << ": image size changed" << std::endl;
            break;
        }
        std::cout << "Frame number: " << i << "\r" << std::flush;
        if (!labels_dir.empty() && (i == 0 || load_image(label_name(i), labels, err))) {  // (frame 0's are loaded; a missing file: no labels for the frame)
            if (labels.w != label_cfg.label_width || labels.h != label_cfg.label_height || !vo->frame_labels(labels.px.data())) {
                std::cout << "frame " << i << ": labels of another size, or refused: " << vo->last_error() << std::endl;
                break;
            }
        }
        const auto t0 = std::chrono::steady_clock::now();
        const bool queued = vo->track_async(lvt_image_view(left.px.data(), left.h, left.w), lvt_image_view(right.px.data(), right.h, right.w));
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!queued) break;
        have = i + 1 < frame_count && load_gray(stem(0, i + 1), nleft, err) && load_gray(stem(1, i + 1), nright, err);  // (an unreadable frame ends the run)
        const auto t1 = std::chrono::steady_clock::now();
        const lvt_pose pose = vo->wait_pose();
        dt += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        total_time += dt;  // (time spent inside the tracker's calls, as the reference reports it)
        if (cov_file.is_open()) {
            lvt_amd_pose_info info;
            vo->get_pose_info(info);
            cov_file << i << " " << info.status << " " << info.n_inliers;
            for (int k = 0; k < 6; k++) cov_file << " " << (info.status == 1 ? std::sqrt(info.cov[7 * k]) : 0.0);
            cov_file << std::endl;
        }
        const lvt_vector3 pos = pose.get_position();  // kitti_example.cpp:40-47
        const lvt_matrix33 R = pose.get_orientation_matrix();
        for (int r = 0; r < 3; r++) {
            rows.push_back(R(r, 0)), rows.push_back(R(r, 1)), rows.push_back(R(r, 2));
            rows.push_back(pos(r));
        }
        n++;
        if (vo->get_state() == lvt_system::eState_LOST) break;
        if (have) std::swap(left, nleft), std::swap(right, nright);
    }
    std::ofstream file(out_name.c_str());
    file << std::fixed;
    static const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (long i = 0; i < frame_count; i++) {
        const double *row = (i < n) ? &rows[(size_t)i * 12] : identity;
        for (int k = 0; k < 12; k++) file << std::setprecision(9) << row[k] << (k == 11 ? "" : " ");
        file << std::endl;
    }
    file.close();
    lvt_system::destroy(vo);
    std::cout << std::endl << "Frames: " << n << "/" << frame_count << "  Average frame processing time: " << (frame_count ? total_time / (double)frame_count : 0.0) << std::endl;
    return 0;
}
