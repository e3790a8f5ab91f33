"""Inputs of the half-precision feature tests (tests/test_gpu_feature_f16.py): the crafted float32 vector the cast is held to
numpy on, and random finite halves.  numpy's astype(float16) IS the reference of the cast; nothing is restated here."""
import numpy as np


def crafted_floats() -> np.ndarray:
    """float32 values around everything the rounding can get wrong: signed zeros, every tie at the 11-bit boundary next to 1.0 and
    2048.0 (odd and even neighbours) and the floats either side of each tie, the overflow threshold, the subnormal halves and
    their ties, float32 subnormals, NaN and the infinities"""
    f32 = np.float32
    v = [0.0, -0.0]
    for base, below, above in ((1.0, 2.0 ** -12, 2.0 ** -11), (2048.0, 0.5, 1.0)):      # half spacing: 2 * below under, 2 * above over
        for k in range(0, 9):
            for x in (base + k * above, base - k * below):                                # odd k: a tie between two halves
                x = f32(x)
                v += [x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))]
    for x in (65504.0, 65519.996, 65520.0, 1e6, 65535.0, 3.0e38):
        x = f32(x)
        v += [x, -x, np.nextafter(x, f32(0)), -np.nextafter(x, f32(0))]
    tiny = [2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, 5 * 2.0 ** -25, 1023 * 2.0 ** -24, 1023.5 * 2.0 ** -24,
            (2.0 ** -14) - 2.0 ** -25, 511.5 * 2.0 ** -24, 512.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 3.5 * 2.0 ** -24]
    for x in tiny:
        x = f32(x)
        for y in (x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(0))):
            v += [y, -y]
    v += [f32(1e-40), f32(-1e-40), np.nextafter(f32(0), f32(1)), -np.nextafter(f32(0), f32(1)), f32(1.17549421e-38)]
    v += [np.nan, -np.nan, np.inf, -np.inf]
    out = np.asarray(v, dtype=np.float32)
    bits = np.asarray([0x7f800001, 0xffc12345, 0x7f801fff, 0x7fffe000], dtype=np.uint32).view(np.float32)     # NaN payloads
    return np.concatenate([out, bits])


def cast_inputs(seed: int = 0) -> np.ndarray:
    """the crafted vector, then 4096 seeded normals scaled by 10^k for k = -8 ... 5"""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(4096).astype(np.float32)
    return np.concatenate([crafted_floats()] + [(n * np.float32(10.0 ** k)).astype(np.float32) for k in range(-8, 6)])


def to_half(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def overflow_count(x: np.ndarray) -> int:
    """finite inputs whose numpy half is not finite"""
    return int((np.isfinite(x) & ~np.isfinite(to_half(x))).sum())


def random_halves(shape, seed: int) -> np.ndarray:
    """uniform random bit patterns of finite halves: normals of every exponent, subnormals, both zeros"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 16, size=shape, dtype=np.uint32).astype(np.uint16)
    bits[(bits & 0x7c00) == 0x7c00] &= 0x83ff                                             # inf / NaN -> subnormals
    return bits.view(np.float16)
