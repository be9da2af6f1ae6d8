"""Writes tests/golden/jpeg_enc/: the seeded pictures of tests/jpeg_enc_model.py (noise and a smooth ramp) encoded by Pillow's libjpeg-turbo
(baseline, optimize=False), the files the forward path of the encoder is held to, coefficient for coefficient
(tests/test_jpeg_enc_cpu.py).  Needs Pillow; run from the repository root:

    python tests/golden/make_jpeg_enc.py
"""
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from PIL import Image  # noqa: E402

from tests import jpeg_enc_model as m  # noqa: E402


def pillow_bytes(kind, w, h, layout, q) -> bytes:
    bgr = m.picture(kind, w, h, grey=layout == "grey")
    buf = io.BytesIO()
    if layout == "grey":
        Image.fromarray(bgr[:, :, 0], "L").save(buf, "JPEG", quality=q, optimize=False)
    else:
        Image.fromarray(bgr[:, :, ::-1].copy(), "RGB").save(buf, "JPEG", quality=q, subsampling=m.SUBSAMPLING[layout], optimize=False)
    return buf.getvalue()


def main():
    os.makedirs(m.FIXTURES, exist_ok=True)
    total = 0
    for case in m.cases():
        data = pillow_bytes(*case)
        with open(os.path.join(m.FIXTURES, m.case_name(*case)), "wb") as f:
            f.write(data)
        total += len(data)
    print(f"{len(m.cases())} files, {total} bytes")


if __name__ == "__main__":
    main()
