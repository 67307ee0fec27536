// lvt_tum -- TUM RGB-D command line harness over the C-ABI.
//
// Same argv, inputs and outputs as the reference's example binary (examples/tum_rgbd/tum_rgbd_example.cpp:49-150 there):
//     lvt_tum <tum_sequences_root_dir> <associations_dir> <dataset_name> <config_file_name> [--max-frames N] [--out name.txt] [--mask FILE]
//                [--depth-guard [R,N,ABS,REL]]
// reads <associations_dir>/<dataset_name>.txt ("t_rgb rgb/xxx.png t_depth depth/xxx.png" per line), the colour and the 16-bit
// depth PNGs below <root>/<dataset_name>/, hands the decoded RGB to the tracker as it is (LVT_AMD_PIX_RGB8: the conversion to gray, cv::cvtColor's
// weights, is the first launch of the frame's feature stage; a dataset of gray PNGs goes in as gray) and the PNG's 16-bit depth plane to
// lvt_amd_track_rgbd16_async with 1.0f / 5000.0f metres per unit (the tracker computes value * (1.0f / 5000.0f) in float where it has key
// points -- what cv::Mat::convertTo gives the reference for every pixel) and writes <dataset_name>.txt in
// the TUM trajectory format "t x y z qx qy qz qw" with the reference's precision (6 digits for t, 7 for the rest).
// --mask FILE (not in the reference): a feature mask (lvt_amd_set_mask), an 8-bit PNG or PGM of the configured image size, a pixel != 0: key points allowed.
// A file of another size is refused before the first frame.
// --depth-guard R,N,ABS,REL (not in the reference): a depth guard (lvt_amd_set_depth_guard): key points whose depth sample has fewer than N of the
// (2R+1)^2 - 1 samples around it valid and within ABS + REL * depth metres of it are dropped.  The bare flag gives lvt_amd_depth_guard_default's record
// (1,4,0.01,0.02).  A record outside its ranges is refused before the first frame.
#include "../include/lvt_amd_ext.h"
#include "../include/lvt_c.h"
#include "image_io.h"

#include <chrono>
#include <cstdio>
#include <iomanip>
#include <iostream>
#include <sstream>

using namespace lvt_io;

int main(int argc, char **argv) {
    if (argc < 5) {
        std::cout << "Usage ./lvt_tum tum_sequences_root_dir associations_dir dataset_name config_file_name [--max-frames N] [--out name.txt]" << std::endl;
        return -1;
    }
    const std::string root_dir = argv[1], associations_dir = argv[2], dataset_name = argv[3], config_file_name = argv[4];
    std::string out_name = dataset_name + ".txt", mask_name;
    long max_frames = -1;
    bool guarded = false;
    lvt_amd_depth_guard guard;
    lvt_amd_depth_guard_default(&guard);
    for (int i = 5; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--depth-guard") {  // (the one option whose value may be left out)
            guarded = true;
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) {
                if (std::sscanf(argv[i + 1], "%d,%d,%f,%f", &guard.radius, &guard.min_support, &guard.tol_abs, &guard.tol_rel) != 4) {
                    std::cout << "--depth-guard takes R,N,ABS,REL (got " << argv[i + 1] << ")" << std::endl;
                    return -1;
                }
            } else {
                i--;
            }
            continue;
        }
        if (i + 1 >= argc) break;
        if (k == "--out") out_name = argv[i + 1];
        else if (k == "--max-frames") max_frames = std::atol(argv[i + 1]);
        else if (k == "--mask") mask_name = argv[i + 1];
    }
    std::vector<std::string> rgb_titles, depth_titles;
    std::vector<double> time_stamps;
    {
        const std::string path = associations_dir + "/" + dataset_name + ".txt";
        std::ifstream f(path);
        if (!f.is_open()) {
            std::cout << "Unable to open asscoiations files " << path << std::endl;
            return -1;
        }
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::stringstream ss(line);
            double t = 0, t2 = 0;
            std::string rgb, depth;
            if (!(ss >> t >> rgb >> t2 >> depth)) continue;
            time_stamps.push_back(t);
            rgb_titles.push_back(rgb);
            depth_titles.push_back(depth);
        }
    }
    if (rgb_titles.empty()) {
        std::cout << "Image asscoiations was not read correctly" << std::endl;
        return -1;
    }
    lvt_amd_params params;
    if (!lvt_amd_params_from_file(config_file_name.c_str(), &params)) {
        std::cout << "Failed to initialize from " << config_file_name << std::endl;
        return -1;
    }
    lvt_handle vo = lvt_amd_create(&params, 2 /* RGBD */);
    if (!vo) {
        std::cout << "failed to create the tracker: " << lvt_amd_last_error(nullptr) << std::endl;
        return -1;
    }
    if (!mask_name.empty()) {
        Gray mask;
        std::string err;
        if (!load_image(mask_name, mask, err)) {
            std::cout << "failed to read the mask " << mask_name << " (" << err << ")" << std::endl;
            return -1;
        }
        if (mask.w != params.img_width || mask.h != params.img_height) {
            std::cout << "the mask " << mask_name << " is " << mask.w << " x " << mask.h << ", the frames are " << params.img_width << " x " << params.img_height << std::endl;
            return -1;
        }
        if (lvt_amd_set_mask(vo, mask.px.data(), nullptr) != 0) {
            std::cout << "failed to set the mask: " << lvt_amd_last_error(vo) << std::endl;
            return -1;
        }
    }
    if (guarded && lvt_amd_set_depth_guard(vo, &guard) != 0) {
        std::cout << "failed to set the depth guard: " << lvt_amd_last_error(vo) << std::endl;
        return -1;
    }
    long frame_count = (long)rgb_titles.size();
    if (max_frames >= 0 && max_frames < frame_count) frame_count = max_frames;
    const float depth_scale = 1.0f / 5000.0f;  // depth values in TUM are scaled
    std::vector<double> poses;                 // q (w x y z), p per processed frame
    double total_time = 0;
    long n = 0;
    // frame i is enqueued (lvt_amd_track_rgbd16_async: pageable buffers are the library's copy when the call returns), frame i + 1 is read and decoded
    // while it tracks, then frame i's pose is collected -- the reference's loop (tum_rgbd_example.cpp:83-103) does the two in turn
    struct Frame {
        Gray rgb, depth;  // (depth.px16: the PNG's 16-bit plane as it is)
        bool ok = false;
    };
    auto load = [&](long i, Frame &f) {
        std::string err;
        f.ok = i < frame_count && load_image(root_dir + "/" + dataset_name + "/" + rgb_titles[i], f.rgb, err) &&
               load_image(root_dir + "/" + dataset_name + "/" + depth_titles[i], f.depth, err) && !f.depth.px16.empty() && f.depth.w == f.rgb.w &&
               f.depth.h == f.rgb.h;
    };
    Frame cur, nxt;
    load(0, cur);
    const bool colour = cur.ok && !cur.rgb.rgb.empty();  // colour PNGs: the tracker takes the interleaved RGB; every later frame must be colour too
    if (colour && lvt_amd_set_pixel_format(vo, LVT_AMD_PIX_RGB8) != 0) {
        std::cout << "failed to set the pixel format: " << lvt_amd_last_error(vo) << std::endl;
        return -1;
    }
    for (long i = 0; i < frame_count; i++) {
        std::cout << "Frame number: " << i << "/" << frame_count << "\r" << std::flush;
        if (!cur.ok) {
            std::cout << "Failed to load image " << std::endl;
            break;
        }
        if (!cur.rgb.rgb.empty() != colour) {  // the pixel format was set from the first frame
            std::cout << "Frame " << i << " is a " << (colour ? "gray" : "colour") << " image in a dataset that began with " << (colour ? "colour" : "gray") << " images" << std::endl;
            break;
        }
        const auto t0 = std::chrono::steady_clock::now();
        const int queued = lvt_amd_track_rgbd16_async(vo, colour ? cur.rgb.rgb.data() : cur.rgb.px.data(), cur.depth.px16.data(), depth_scale, cur.rgb.h, cur.rgb.w);
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (queued != 0) break;  // (a frame of another size: the reference would throw inside OpenCV)
        load(i + 1, nxt);
        const auto t1 = std::chrono::steady_clock::now();
        double q[4], p[3];
        const int state = lvt_amd_wait_pose(vo, q, p);
        total_time += dt + std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        for (int k = 0; k < 4; k++) poses.push_back(q[k]);
        for (int k = 0; k < 3; k++) poses.push_back(p[k]);
        n++;
        if (state == 3) break;  // LOST
        std::swap(cur, nxt);
    }
    std::ofstream file(out_name.c_str());
    file << std::fixed;
    for (long i = 0; i < (long)rgb_titles.size(); i++) {  // one row per association line, default pose after the end / a LOST
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
    std::cout << std::endl << "Frames: " << n << "/" << frame_count << "  Average frame processing time: " << (n ? total_time / (double)n : 0.0) << std::endl;
    return 0;
}
