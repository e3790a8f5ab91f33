"""acx_jpeg_entropy_encode_dev, the Huffman coder of the qualitative videos' frames on the device, against the host coder
acx_jpeg_entropy_encode on the same coefficients: byte for byte the same files, the same sizes, the same codes.  Everything is
exact: there are no tolerances."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_encode_dev_cases as EC
import jpeg_restated as JR
from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops
from anomalyclip_amd import visualizer as V

DEV = torch.device("cuda", 0)
OK, E_BADARG, E_WORKSPACE = 0, -1, -4
SENTINEL = 0xA5
SMALL = [(16, 16), (48, 32), (33, 47)]                   # 6, 36 and 54 blocks
LARGE = [(176, 208), (304, 400)]                         # 858 blocks: no multiple of 64 or 256; 2,850: more than 1,024
QT = V.quant_tables(90)


def header_dev(H, W):
    return torch.from_numpy(ops.jpeg_encode_header(QT, H, W)).to(DEV)


def encode(frames, H, W, cap=None, workspace=None):
    """the device coder on the frames [(name, coef)] -> (slots uint8 [B, cap + 64] as they are afterwards, nbytes, status); every
    slot lies in a buffer of sentinel bytes with 64 more behind the last, which must survive"""
    B = len(frames)
    coef = torch.from_numpy(np.stack([c for _, c in frames])).to(DEV)
    cap = ops.jpeg_encode_bound(H, W) if cap is None else cap
    buf = torch.full((B * cap + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    files, nbytes, status = ops.jpeg_entropy_encode_dev(coef, header_dev(H, W), H, W, cap=cap, files=buf[:B * cap], workspace=workspace)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[B * cap:] == SENTINEL).all(), "bytes behind the last slot were written"
    return out[:B * cap].reshape(B, cap), nbytes.cpu().numpy(), status.cpu().numpy()


def check_equal(frames, H, W, slots, nbytes, status, want=None):
    """every frame's slot holds the host coder's file and sentinel bytes behind it"""
    want = [EC.host_file(c, QT, H, W) for _, c in frames] if want is None else want
    for f, ((name, _), w) in enumerate(zip(frames, want)):
        assert isinstance(w, bytes), name
        assert (int(status[f]), int(nbytes[f])) == (OK, len(w)), (name, H, W)
        assert slots[f, :len(w)].tobytes() == w, (name, H, W)
        assert (slots[f, len(w):] == SENTINEL).all(), (name, H, W, "bytes behind the file were written")
    return want


@pytest.mark.parametrize("H,W", SMALL)
def test_small_frames_equal_the_host_coder(H, W):
    """each case alone (B = 1), then all of them in one launch: frames of 6 bits a block beside frames of 1,658; and the host
    parser and decoder give the coefficients back from a device-made file"""
    cases = EC.all_cases(H, W)
    assert len(cases) >= 7
    want = [EC.host_file(c, QT, H, W) for _, c in cases]
    for case, w in zip(cases, want):
        check_equal([case], H, W, *encode([case], H, W), want=[w])
    slots, nbytes, status = encode(cases, H, W)
    check_equal(cases, H, W, slots, nbytes, status, want=want)
    assert max(nbytes) - 625 > 20 * (min(nbytes) - 625)                          # (the scans, without header and EOI)
    for f, (name, c) in enumerate(cases):
        rc, geom, back, qt = JR.host_decode(slots[f, :nbytes[f]].tobytes())
        assert rc == OK and (geom["H"], geom["W"], geom["hs"], geom["vs"]) == (H, W, 2, 2), name
        assert np.array_equal(back, c) and np.array_equal(qt[0], QT[0]) and np.array_equal(qt[1], QT[1]), name


@pytest.mark.parametrize("H,W", LARGE)
def test_large_frames_equal_the_host_coder(H, W):
    """all zero, dense, sparse and maximal in one launch (B = 4); the maximal frame's blocks have 1,658 bits where they are luma"""
    cases = EC.large_cases(H, W)
    slots, nbytes, status = encode(cases, H, W)
    want = check_equal(cases, H, W, slots, nbytes, status)
    nb = len(cases[0][1]) // 64
    assert len(want[3]) > nb * 4 // 6 * EC.MAX_BLOCK_BITS // 8                   # (the luma blocks alone)
    assert want[1].count(b"\xff\x00") > 100                                      # the dense frame's scan is stuffed
    rc, _, back, _ = JR.host_decode(slots[3, :nbytes[3]].tobytes())
    assert rc == OK and np.array_equal(back, cases[3][1])


def test_capacity():
    """cap equal to the largest file: every frame fits; one byte less: ACX_E_WORKSPACE for exactly the frames that do not, their
    nbytes still the size they need, no byte at or past any slot's end"""
    H, W = 48, 32
    cases = EC.all_cases(H, W)
    want = [EC.host_file(c, QT, H, W) for _, c in cases]
    sizes = np.array([len(w) for w in want])
    cap = int(sizes.max())
    check_equal(cases, H, W, *encode(cases, H, W, cap=cap), want=want)
    slots, nbytes, status = encode(cases, H, W, cap=cap - 1)
    assert np.array_equal(nbytes, sizes)
    assert np.array_equal(status, np.where(sizes > cap - 1, E_WORKSPACE, OK)) and (status == E_WORKSPACE).sum() >= 1 and (status == OK).sum() >= 1
    for f, w in enumerate(want):
        n = min(len(w), cap - 1)
        assert slots[f, :n].tobytes() == w[:n] and (slots[f, n:] == SENTINEL).all(), cases[f][0]
    # a slot that holds not even the header
    slots, nbytes, status = encode(cases, H, W, cap=100)
    assert np.array_equal(nbytes, sizes) and (status == E_WORKSPACE).all()
    assert all(slots[f].tobytes() == w[:100] for f, w in enumerate(want))


def test_refusals():
    """a DC difference of category 12 and an AC of 1024 among good frames: ACX_E_BADARG for those two alone, their slots left as
    they were; the bad arguments are a code before any launch"""
    H, W = 48, 32
    good = EC.large_cases(H, W)
    dc = good[2][1].copy()
    dc[0], dc[64] = -2047, 2047                                                  # the first two luma blocks of the scan
    ac = good[2][1].copy()
    ac[-64 + 5] = 1024
    frames = [good[0], ("DC difference of category 12", dc), good[1], good[3], ("AC 1024", ac), good[2]]
    assert EC.host_file(dc, QT, H, W) == E_BADARG and EC.host_file(ac, QT, H, W) == E_BADARG
    slots, nbytes, status = encode(frames, H, W)
    assert status.tolist() == [OK, E_BADARG, OK, OK, E_BADARG, OK]
    assert nbytes[1] == 0 and nbytes[4] == 0 and (slots[1] == SENTINEL).all() and (slots[4] == SENTINEL).all()
    keep = [0, 2, 3, 5]
    check_equal([frames[f] for f in keep], H, W, slots[keep], nbytes[keep], status[keep])

    lib, h = L.lib(), L.ctx(0)
    B = 2
    coef = torch.zeros(B, R_elems(H, W), dtype=torch.int16, device=DEV)
    head = header_dev(H, W)
    cap = ops.jpeg_encode_bound(H, W)
    files = torch.full((B * cap,), SENTINEL, dtype=torch.uint8, device=DEV)
    res = torch.full((2, B), 77, dtype=torch.int32, device=DEV)
    need = ops.jpeg_entropy_encode_dev_workspace_bytes(H, W, B)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(coef=coef.data_ptr(), header=head.data_ptr(), hb=head.numel(), H=H, W=W, B=B, files=files.data_ptr(), cap=cap,
                 nbytes=res[0].data_ptr(), status=res[1].data_ptr(), ws=ws.data_ptr(), wsb=need)
        a.update(kw)
        return lib.acx_jpeg_entropy_encode_dev(h, a["coef"], a["header"], a["hb"], a["H"], a["W"], a["B"], a["files"], a["cap"],
                                               a["nbytes"], a["status"], a["ws"], a["wsb"], stream)

    for key in ("coef", "header", "files", "nbytes", "status", "ws"):
        assert call(**{key: None}) == E_BADARG, key
    assert call(B=0) == E_BADARG and call(B=-1) == E_BADARG and call(H=0) == E_BADARG and call(W=65536) == E_BADARG
    assert call(hb=0) == E_BADARG and call(cap=-1) == E_BADARG
    assert call(H=65535, W=833) == E_BADARG                                      # 1,302,528 blocks x 1,658 bits pass 2^31
    assert call(wsb=need - 1) == E_WORKSPACE
    assert lib.acx_jpeg_entropy_encode_dev_workspace_bytes(0, W, B) == 0 and lib.acx_jpeg_entropy_encode_dev_workspace_bytes(H, 65536, B) == 0
    assert lib.acx_jpeg_entropy_encode_dev_workspace_bytes(H, W, 0) == 0 and lib.acx_jpeg_entropy_encode_dev_workspace_bytes(65535, 833, 1) == 0
    torch.cuda.synchronize()
    assert (files.cpu().numpy() == SENTINEL).all() and (res.cpu().numpy() == 77).all(), "a refused call launched something"
    assert call() == OK
    torch.cuda.synchronize()
    assert res[1].cpu().tolist() == [OK, OK]


def R_elems(H, W):
    return ops.jpeg_coef_elems(H, W, 3, 2, 2)


def test_workspace_reuse():
    """two calls on one workspace and one stream, dense frames and then sparse ones of the same size, without a host wait between
    them: both right (the second call merges into words the first one left full)"""
    H, W = 176, 208
    by_name = dict(EC.large_cases(H, W))
    B = 2
    ws = torch.empty(ops.jpeg_entropy_encode_dev_workspace_bytes(H, W, B), dtype=torch.uint8, device=DEV)
    ws.fill_(0xFF)
    head = header_dev(H, W)
    cap = ops.jpeg_encode_bound(H, W)
    outs = []
    for name in ("maximal blocks", "dense", "sparse", "all zero"):
        coef = torch.from_numpy(np.stack([by_name[name]] * B)).to(DEV)
        files = torch.full((B, cap), SENTINEL, dtype=torch.uint8, device=DEV)
        outs.append((name, *ops.jpeg_entropy_encode_dev(coef, head, H, W, cap=cap, files=files, workspace=ws)))
    torch.cuda.synchronize()
    for name, files, nbytes, status in outs:
        frames = [(name, by_name[name])] * B
        check_equal(frames, H, W, files.cpu().numpy(), nbytes.cpu().numpy(), status.cpu().numpy())
