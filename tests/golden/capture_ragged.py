"""Writes tests/golden/r1_ragged_jpeg.npz: JPEG files of DIFFERENT sizes and sampling factors encoded by Pillow from seeded
synthetic images, with PILLOW'S decoded pixels as the expected output - the pin of the ragged decode + resize path
(DeviceJpegDecoder.decode_ragged / DeviceResize on RaggedImages, editor_jpeg_reconstruct_ragged / editor_resize_u8_ragged):
the separate-file sample layout of RGBNT201 / MSVR310, where every modality is a detector crop of its own size
(data/datasets/bases.py:22-30).  The sizes are the smallest at which the per-image indexing can go wrong; all are at least 7x9
(narrower subsampled files take libjpeg's plain chroma upsampler, which the decoder does not restate: DESIGN.md 6).
Run in the build container (Pillow 12.2.0, libjpeg-turbo):  python tests/golden/capture_ragged.py"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [  # (name, W, H, subsampling | 'gray', quality, extra save options)
    ("a_odd_420_7x9", 7, 9, 2, 75, {}),                     # partial MCUs on both edges, upscaled in both axes by every target
    ("b_odd_422_15x17", 15, 17, 1, 85, {}),
    ("c_odd_444_17x33", 17, 33, 0, 90, {}),
    ("d_odd_420_97x211", 97, 211, 2, 60, {}),
    ("e_mcu_444_8x8", 8, 8, 0, 80, {}),                     # exactly one MCU
    ("f_mcu_420_16x16", 16, 16, 2, 80, {}),
    ("g_gray_45x61", 45, 61, "gray", 80, {}),
    ("h_prog_420_53x47", 53, 47, 2, 75, dict(progressive=True)),
    ("i_restart_422_75x40", 75, 40, 1, 80, dict(restart_marker_blocks=3)),
    ("j_wout_420_128x90", 128, 90, 2, 75, {}),              # exactly Wout wide for the 256x128 target: horizontal pass is a copy
    ("k_hout_422_200x256", 200, 256, 1, 70, {}),            # exactly Hout tall: vertical pass is a copy
    ("l_exact_444_128x256", 128, 256, 0, 70, {}),           # exactly the target: both passes are copies
    ("m_wide_420_321x173", 321, 173, 2, 65, {}),            # much larger in one axis: the widest tap tables of the batch
    ("n_odd_444_33x71", 33, 71, 0, 75, dict(optimize=True)),
]


def synth(rng, w, h, gray):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 128 + 90 * np.cos(xx / 29.0 + yy / 7.0),
                     255.0 * (xx + yy) / (w + h)], axis=2)
    base += rng.normal(0, 12, base.shape)
    a = np.clip(base, 0, 255).astype(np.uint8)
    return Image.fromarray(a[..., 0] if gray else a)


def main():
    rng = np.random.default_rng(21)
    out = {}
    for name, w, h, ss, q, kw in CASES:
        im = synth(rng, w, h, ss == "gray")
        bio = io.BytesIO()
        if ss == "gray":
            im.save(bio, "JPEG", quality=q, **kw)
        else:
            im.save(bio, "JPEG", quality=q, subsampling=ss, **kw)
        data = bio.getvalue()
        out[name + ".jpg"] = np.frombuffer(data, dtype=np.uint8)
        out[name + ".rgb"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert out[name + ".rgb"].shape == (h, w, 3)
    path = os.path.join(HERE, "r1_ragged_jpeg.npz")
    np.savez_compressed(path, **out)
    print("wrote r1_ragged_jpeg.npz: %d bytes" % os.path.getsize(path), {k: v.shape for k, v in out.items() if k.endswith(".rgb")})


if __name__ == "__main__":
    main()
