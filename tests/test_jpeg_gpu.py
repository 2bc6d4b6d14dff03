"""GPU: ssd_jpeg_reconstruct (dequantise, IDCT, chroma upsampling, colour) and ops.decode_jpeg_batch against the committed
Pillow decode of the fixtures, bit for bit, in a poisoned arena with guard bands (tests/strict.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import jpeg_cases as C                                      # noqa: E402
from tests import strict as S                                          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _records(names):
    """(coef int16 [total], desc int32 [B, REC]) of the oracle's coefficients, offsets absolute"""
    return _records_of([C.oracle(name) for name in names])


def _records_of(pairs):
    """_records of (coefficients, header) pairs"""
    from ssd_object_detection_amd import _lib
    g = _lib.CONSTANTS
    coefs, desc, base = [], np.zeros((len(pairs), g["SSD_JPEG_REC_WORDS"]), np.int32), 0
    for b, (coef, h) in enumerate(pairs):
        r = desc[b]
        r[g["SSD_JPEG_WIDTH"]], r[g["SSD_JPEG_HEIGHT"]], r[g["SSD_JPEG_NCOMP"]] = h["width"], h["height"], h["ncomp"]
        r[g["SSD_JPEG_KIND"]], r[g["SSD_JPEG_NCOEF"]], r[g["SSD_JPEG_RESTART"]] = h["kind"], h["ncoef"], h["restart"]
        for c in range(h["ncomp"]):
            r[g["SSD_JPEG_BLOCKS_W"] + c], r[g["SSD_JPEG_BLOCKS_H"] + c] = h["blocks_w"][c], h["blocks_h"][c]
            r[g["SSD_JPEG_COEF_OFF"] + c] = base + h["coef_off"][c]
            r[g["SSD_JPEG_QT"] + 64 * c:][:64] = h["qt"][c]
        coefs.append(coef)
        base += h["ncoef"]
    return np.concatenate(coefs), desc


def _reconstruct_strict(names):
    """one ssd_jpeg_reconstruct call for `names` into per-image slots of a poisoned arena: every image equals Pillow's decode,
    every guard byte (1 MiB in front of and behind each image, the coefficients, the records and the scratch) is intact, the
    inputs are unchanged, and nothing depends on what the scratch or the arena held before"""
    _reconstruct_strict_of([C.oracle(n) for n in names], [C.decoded(n) for n in names], names)


def _reconstruct_strict_of(pairs, images, names):
    from ssd_object_detection_amd import ops
    coef, desc = _records_of(pairs)
    want = [torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()) for img in images]
    arena = S.Arena(DEV, S.Arena.bytes_for(coef.nbytes, desc.nbytes, 8 * len(names), coef.size, *[w.numel() for w in want]))
    coef_d = arena.put(torch.from_numpy(coef), "coef")
    desc_d = arena.put(torch.from_numpy(desc), "desc")
    outs = [arena.out((w.numel(),), torch.uint8, "image %d %s" % (i, n)) for i, (n, w) in enumerate(zip(names, want))]
    off = torch.tensor([o.data_ptr() - arena.buf.data_ptr() for o in outs], dtype=torch.int64)
    off_d = arena.put(off, "dst_off")
    scratch = arena.workspace().get(coef.size, DEV)
    arena.run(lambda: ops.jpeg_reconstruct(coef_d, desc_d, arena.buf, off_d, scratch=scratch), list(zip(outs, want)))


def test_reconstruct_ragged_batch_is_pillow_bit_for_bit():
    _reconstruct_strict(list(C.SUPPORTED))


def test_reconstruct_reversed_batch():
    _reconstruct_strict(list(C.SUPPORTED)[::-1])


def test_reconstruct_single_pixel_image():
    _reconstruct_strict(["c1x1"])


@pytest.mark.parametrize("key", sorted(C.LARGE))
def test_reconstruct_past_one_stride_of_the_loops(key):
    """jpeg_cases.LARGE: a fixture's blocks repeated to more than 16 384 blocks (4:4:4: k_jpeg_idct's second trip) and more than
    32 768 pixels (k_jpeg_rgb's: eleven and three trips), against the numpy oracle's reconstruction of the same coefficients;
    a small fixture rides in the same call"""
    from tests import jpeg_oracle as J
    coef, h = C.tiled(*C.LARGE[key])
    blocks, pixels = coef.size // 64, h["width"] * h["height"]
    print(key, blocks, "blocks,", pixels, "pixels")
    assert pixels > 2 * C.RGB_STRIDE and (key != "444" or blocks > C.IDCT_STRIDE)
    small = "c17x9_420"
    _reconstruct_strict_of([(coef, h), C.oracle(small)], [J.reconstruct(coef, h), C.decoded(small)], [key, small])


def test_reconstruct_refuses_bad_arguments_and_skips_bad_records():
    from ssd_object_detection_amd import _lib, ops
    names = ["c17x9_420", "c33x20_grey", "c31x16_422"]
    coef, desc = _records(names)
    g = _lib.CONSTANTS
    sizes = [C.decoded(n).size for n in names]
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    coef_d, off_d = torch.from_numpy(coef).to(DEV), torch.from_numpy(off).to(DEV)
    dst = torch.full((sum(sizes),), 0xA5, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):                                  # scratch one byte short: SSD_ERR_WORKSPACE
        ops.jpeg_reconstruct(coef_d, torch.from_numpy(desc).to(DEV), dst, off_d,
                             scratch=torch.empty(coef.size - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):                                    # a coefficient count that is no multiple of 64
        ops.jpeg_reconstruct(coef_d[:-1].clone(), torch.from_numpy(desc).to(DEV), dst, off_d)
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    # records the kernels must not follow: planes past the coefficients, a grid that does not cover the image, a destination
    # past the arena.  Each writes nothing; the other images still come out right
    bad = desc.copy()
    bad[0, g["SSD_JPEG_COEF_OFF"] + 2] = coef.size                     # image 0: the Cr plane starts behind the buffer
    bad[1, g["SSD_JPEG_WIDTH"]] = 8 * bad[1, g["SSD_JPEG_BLOCKS_W"]] + 1       # image 1: wider than its plane
    ops.jpeg_reconstruct(coef_d, torch.from_numpy(bad).to(DEV), dst, off_d)
    got = dst.cpu().numpy()
    assert (got[:off[2]] == 0xA5).all()
    assert np.array_equal(got[off[2]:], C.decoded(names[2]).reshape(-1))
    dst.fill_(0xA5)
    far = off.copy()
    far[2] = dst.numel() - sizes[2] + 1                                # image 2 would end one byte behind the arena
    ops.jpeg_reconstruct(coef_d, torch.from_numpy(desc).to(DEV), dst, torch.from_numpy(far).to(DEV))
    got = dst.cpu().numpy()
    assert np.array_equal(got[:off[1]], C.decoded(names[0]).reshape(-1)) and (got[off[2]:] == 0xA5).all()


def _expected_arena(names):
    return np.concatenate([C.decoded(n).reshape(-1) for n in names])


def test_decode_jpeg_batch_equals_pillow():
    from ssd_object_detection_amd import ops
    names = list(C.SUPPORTED)
    arena, off, hw, stats = ops.decode_jpeg_batch([C.data(n) for n in names], DEV)
    assert stats.fallback == 0 and stats.images == stats.device == len(names)
    assert arena.dtype == torch.uint8 and off.dtype == torch.int64 and hw.dtype == torch.int32
    assert hw.cpu().tolist() == [list(C.decoded(n).shape[:2]) for n in names]
    sizes = [C.decoded(n).size for n in names]
    assert off.cpu().tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    assert np.array_equal(arena.cpu().numpy(), _expected_arena(names))
    # the arena is what image_resize_prep takes
    x = ops.image_resize_prep(arena, off, hw, 300, True)
    flat = torch.from_numpy(_expected_arena(names)).to(DEV)
    assert torch.equal(x, ops.image_resize_prep(flat, off, hw, 300, True))


def test_decode_jpeg_batch_workers_and_reuse():
    from ssd_object_detection_amd import ops
    names = list(C.SUPPORTED) * 3
    enc = [C.data(n) for n in names]
    a1 = ops.decode_jpeg_batch(enc, DEV, workers=1)[0]
    a4 = ops.decode_jpeg_batch(enc, DEV, workers=4)[0]
    small = ops.decode_jpeg_batch(enc[:2], DEV, workers=4)[0]          # the staging buffer is reused: a1, a4 stay as they were
    assert torch.equal(a1, a4) and np.array_equal(a1.cpu().numpy(), _expected_arena(names))
    assert np.array_equal(small.cpu().numpy(), _expected_arena(names[:2]))
    wrapped = ops.decode_jpeg_batch([ops.EncodedImage(C.data(n), *C.decoded(n).shape[:2]) for n in names[:5]], DEV)[0]
    assert np.array_equal(wrapped.cpu().numpy(), _expected_arena(names[:5]))


def test_decode_jpeg_batch_refusals_and_fallback(capsys):
    from ssd_object_detection_amd import ops
    names = ["c17x9_420", "progressive", "c33x20_grey"]
    enc = [C.data(n) for n in names]
    with pytest.raises(NotImplementedError, match="sample 1"):
        ops.decode_jpeg_batch(enc, DEV, fallback=None)
    with pytest.raises(ValueError, match="sample 2"):
        ops.decode_jpeg_batch([enc[0], enc[2], enc[2][:200]], DEV)
    with pytest.raises(ValueError, match="sample 0"):
        ops.decode_jpeg_batch([C.corrupted("c83x61_420_rst")[-1][1], enc[0]], DEV)
    with pytest.raises(ValueError):
        ops.decode_jpeg_batch([], DEV)
    try:
        import PIL  # noqa: F401
    except ImportError:
        with capsys.disabled():
            print("\nPillow is not installed: the fallback's own decode is not checked here")
        with pytest.raises(NotImplementedError, match="Pillow"):
            ops.decode_jpeg_batch(enc, DEV)
        return
    arena, off, hw, stats = ops.decode_jpeg_batch(enc, DEV)
    assert stats.fallback == 1 and stats.device == 2 and stats.images == 3
    assert hw.cpu().tolist() == [list(C.decoded(n).shape[:2]) for n in names]
    assert np.array_equal(arena.cpu().numpy(), _expected_arena(names))


def test_image_arena_takes_a_mix_of_encoded_and_decoded():
    from ssd_object_detection_amd import ops
    names = ["c83x61_444", "c24x40_q1", "c300x2", "c8x8"]
    items = [C.data(names[0]), C.decoded(names[1]), ops.EncodedImage(C.data(names[2]), 2, 300), C.decoded(names[3])]
    arena, off, hw, stats = ops.image_arena(items, DEV)
    assert stats.device == 2 and stats.fallback == 0
    assert np.array_equal(arena.cpu().numpy(), _expected_arena(names))
    assert hw.cpu().tolist() == [list(C.decoded(n).shape[:2]) for n in names]
