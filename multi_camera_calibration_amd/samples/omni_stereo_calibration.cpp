// omni_stereo_calibration -- two-camera omnidirectional calibration on pre-detected corners: read
// the per-view pattern points and both cameras' image points, cv::omnidir::stereoCalibrate with the
// reference sample's TermCriteria(3, 200, 1e-8) (samples/omni_stereo_calibration.cpp:309), and
// write both cameras' parameters, the relative pose, the kept views' poses and the rms.
// Chessboard detection in images is out of scope (the input is the tutorial data format,
// tutorials/data/omni_stereocalib_data.xml: objectPoints, imagePoints1, imagePoints2, imageSize1,
// imageSize2); the calibration runs on the GPU through mcc::omnidir::stereoCalibrate.
//
//   omni_stereo_calibration [-fs] [-fp] [-o out_camera_params_stereo.xml] input.xml
#include <cstdio>
#include <cstring>
#include <ctime>
#include <iostream>
#include <string>
#include <vector>

#include "mcc_omnidir.hpp"
#include "mcc_storage.hpp"

using mcc::storage::FileStorage;
using mcc::storage::Mat;
using mcc::storage::Node;

namespace {

std::vector<Mat> mats(const Node& n) {
    std::vector<Mat> out;
    if (n.type == Node::MAT) out.push_back(n.mat);
    for (const Node& k : n.seq)
        if (k.type == Node::MAT) out.push_back(k.mat);
    return out;
}

std::vector<std::vector<mcc::omnidir::Vec2d>> points2(const std::vector<Mat>& m) {
    std::vector<std::vector<mcc::omnidir::Vec2d>> out(m.size());
    for (size_t v = 0; v < m.size(); ++v)
        for (size_t j = 0; j < m[v].total(); ++j) out[v].push_back({m[v].data[2 * j], m[v].data[2 * j + 1]});
    return out;
}

void write_camera(FileStorage& out, const std::string& suffix, const std::array<double, 9>& K, double xi,
                  const std::array<double, 4>& D) {
    Mat Km(3, 3, 'd'), Dm(1, 4, 'd');
    for (int k = 0; k < 9; ++k) Km.data[k] = K[k];
    for (int k = 0; k < 4; ++k) Dm.data[k] = D[k];
    out.write("camera_matrix_" + suffix, Km);
    out.write("distortion_coefficients_" + suffix, Dm);
    out.write("xi_" + suffix, xi);
}

}  // namespace

int main(int argc, char** argv) {
    std::string input, output = "out_camera_params_stereo.xml";
    int flags = 0;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "-fs")) flags |= mcc::omnidir::CALIB_FIX_SKEW;
        else if (!std::strcmp(argv[i], "-fp")) flags |= mcc::omnidir::CALIB_FIX_CENTER;
        else if (!std::strcmp(argv[i], "-o") && i + 1 < argc) output = argv[++i];
        else input = argv[i];
    }
    if (input.empty()) {
        std::cout << "usage: omni_stereo_calibration [-fs] [-fp] [-o out_camera_params_stereo.xml] corners.xml\n";
        return 0;
    }
    FileStorage fs(input, FileStorage::READ);
    if (!fs.isOpened()) {
        std::cout << "Can not read " << input << std::endl;
        return -1;
    }
    const std::vector<Mat> obj = mats(fs["objectPoints"]), img1 = mats(fs["imagePoints1"]),
                           img2 = mats(fs["imagePoints2"]);
    const Node& sz1 = fs["imageSize1"];
    const Node& sz2 = fs["imageSize2"];
    if (obj.empty() || obj.size() != img1.size() || obj.size() != img2.size() || sz1.seq.size() != 2 ||
        sz2.seq.size() != 2) {
        std::cout << "input needs objectPoints, imagePoints1, imagePoints2 (one matrix per view each), imageSize1 "
                     "and imageSize2"
                  << std::endl;
        return -1;
    }
    std::vector<std::vector<mcc::omnidir::Vec3d>> objectPoints(obj.size());
    for (size_t v = 0; v < obj.size(); ++v)
        for (size_t j = 0; j < obj[v].total(); ++j)
            objectPoints[v].push_back({obj[v].data[3 * j], obj[v].data[3 * j + 1], obj[v].data[3 * j + 2]});
    const auto imagePoints1 = points2(img1), imagePoints2 = points2(img2);
    const mcc::omnidir::Size imageSize1(sz1.seq[0].toInt(), sz1.seq[1].toInt());
    const mcc::omnidir::Size imageSize2(sz2.seq[0].toInt(), sz2.seq[1].toInt());
    std::array<double, 9> K1{}, K2{};
    std::array<double, 4> D1{}, D2{};
    double xi1 = 0, xi2 = 0;
    mcc::omnidir::Vec3d rvec{}, tvec{};
    std::vector<mcc::omnidir::Vec3d> rvecs, tvecs;
    std::vector<int> idx;
    const mcc::omnidir::TermCriteria criteria(3, 200, 1e-8);
    double rms = 0;
    try {
        rms = mcc::omnidir::stereoCalibrate(objectPoints, imagePoints1, imagePoints2, imageSize1, imageSize2, K1, xi1,
                                            D1, K2, xi2, D2, rvec, tvec, rvecs, tvecs, flags, criteria, &idx);
    } catch (const std::exception& e) {
        std::cout << e.what() << std::endl;
        return -1;
    }
    std::cout << "Saving camera params to " << output << std::endl;
    FileStorage out(output, FileStorage::WRITE);
    char buf[256];
    std::time_t tt = std::time(nullptr);
    std::strftime(buf, sizeof(buf) - 1, "%c", std::localtime(&tt));
    out.write("calibration_time", std::string(buf));
    out.write("nFrames", (int)rvecs.size());
    out.write("flags", flags);
    write_camera(out, "1", K1, xi1, D1);
    write_camera(out, "2", K2, xi2, D2);
    Mat rv(3, 1, 'd'), tv(3, 1, 'd'), ext((int)rvecs.size(), 6, 'd'), used(1, (int)idx.size(), 'i');
    for (int k = 0; k < 3; ++k) {
        rv.data[k] = rvec[k];
        tv.data[k] = tvec[k];
    }
    for (size_t i = 0; i < rvecs.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            ext.at((int)i, k) = rvecs[i][k];
            ext.at((int)i, 3 + k) = tvecs[i][k];
        }
    for (size_t i = 0; i < idx.size(); ++i) used.data[i] = idx[i];
    out.write("rvec", rv);   // camera 1 frame -> camera 2 frame
    out.write("tvec", tv);
    out.write("used_imgs", used);              // indices of the views kept by both cameras
    out.write("extrinsic_parameters", ext);    // camera 1's pose of every kept view: rvec, tvec
    out.write("rms", rms);
    out.release();
    std::printf("rms %.9f  om %.9f %.9f %.9f  T %.6f %.6f %.6f  xi1 %.9f xi2 %.9f  views %zu\n", rms, rvec[0], rvec[1],
                rvec[2], tvec[0], tvec[1], tvec[2], xi1, xi2, rvecs.size());
    return 0;
}
