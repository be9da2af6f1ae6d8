// cv::imwrite of shim/cv_compat.h (without OpenCV) on a seeded picture with a padded pitch: tests/test_jpeg_enc_cpu.py compares the files
// with the host encoder's.
//   cv_imwrite_demo <out dir>
#include <cstdio>
#include <string>
#include <vector>

#include "cv_compat.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const int rows = 21, cols = 37;
    const size_t step = cols * 3 + 9;
    std::vector<unsigned char> buf(rows * step, 0xEE);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols * 3; ++x) buf[y * step + x] = (unsigned char)((x * 7 + y * 13 + (x % 3) * 40) & 255);
    const cv::Mat img(rows, cols, CV_8UC3, buf.data(), step);
    const std::string dir = argv[1];
    int bad = 0;
    bad += !cv::imwrite(dir + "/default.jpg", img);
    bad += !cv::imwrite(dir + "/q80_444.JPG", img, {cv::IMWRITE_JPEG_QUALITY, 80, cv::IMWRITE_JPEG_SAMPLING_FACTOR, cv::IMWRITE_JPEG_SAMPLING_FACTOR_444});
    bad += cv::imwrite(dir + "/picture.png", img);                          // not a format this header writes
    bad += cv::imwrite(dir + "/empty.jpg", cv::Mat());
    bad += cv::imwrite(dir + "/no/such/dir.jpg", img);
    const cv::Mat back = cv::imread(dir + "/default.jpg");
    bad += back.rows != rows || back.cols != cols;
    printf("cv_imwrite_demo: %d failures\n", bad);
    return bad ? 1 : 0;
}
