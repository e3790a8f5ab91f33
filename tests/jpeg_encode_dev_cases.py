"""The coefficient frames the device Huffman coder's tests add to viz_ref.entropy_cases, and the host coder as their oracle."""
import numpy as np

import viz_ref as R

MAX_BLOCK_BITS = 20 + 63 * 26          # a DC code of 9 + 11 bits and 63 AC codes of 16 + 10


def scan_order(H: int, W: int) -> np.ndarray:
    """[blocks]: the index, in the coefficient layout, of the block the interleaved 4:2:0 scan visits s-th, and its component"""
    mx, my = -(-W // 16), -(-H // 16)
    order, comp = [], []
    for y in range(my):
        for x in range(mx):
            for v in range(2):
                for h in range(2):
                    order.append((2 * y + v) * 2 * mx + 2 * x + h)
                    comp.append(0)
            for c in (1, 2):
                order.append((3 + c) * mx * my + y * mx + x)
                comp.append(c)
    return np.array(order), np.array(comp)


def maximal_frame(H: int, W: int, every: int = 1) -> np.ndarray:
    """int16 [coef_elems]: every `every`-th block of the scan has all 63 AC at +-1023 and a DC of +-1023 that alternates within
    its component (differences of category 11) -- MAX_BLOCK_BITS bits where the AC table's code has 16; the others are zero"""
    order, comp = scan_order(H, W)
    c = np.zeros((len(order), 64), np.int16)
    sign = [1, 1, 1]
    ac = np.where(np.arange(1, 64) % 2 == 1, -1023, 1023)
    for s, (b, k) in enumerate(zip(order, comp)):
        if s % every == every - 1:
            c[b, 0] = 1023 * sign[k]
            c[b, 1:] = ac
        sign[k] = -sign[k]
    return c.reshape(-1)


def extra_cases(H: int, W: int):
    return [("maximal blocks", maximal_frame(H, W)), ("zero and maximal blocks", maximal_frame(H, W, every=2))]


def all_cases(H: int, W: int):
    return R.entropy_cases(H, W) + extra_cases(H, W)


def large_cases(H: int, W: int):
    """all zero, dense, sparse and maximal"""
    by_name = dict(R.entropy_cases(H, W))
    return [("all zero", by_name["all zero"]), ("dense", by_name["dense random: FF bytes"]), ("sparse", by_name["sparse random"]),
            ("maximal blocks", maximal_frame(H, W))]


def host_file(coef: np.ndarray, qt: np.ndarray, H: int, W: int):
    """the host coder's file, or its negative code"""
    from anomalyclip_amd import ops
    buf = np.empty(ops.jpeg_encode_bound(H, W), np.uint8)
    n = ops.jpeg_entropy_encode(np.ascontiguousarray(coef), qt, H, W, buf)
    return buf[:n].tobytes() if n > 0 else n
