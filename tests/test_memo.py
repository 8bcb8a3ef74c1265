"""neuralbody_amd._memo: the tensor key and the memo behind every host-side cache ("Nothing about a frame lives on the
host"), and what copying or pickling the objects that own one carries."""
import copy
import gc
import pickle
import weakref

import pytest
import torch

from neuralbody_amd import ops
from neuralbody_amd._memo import Memo, tkey
from neuralbody_amd.network import Network
from neuralbody_amd.renderer import RenderConfig, Renderer


class Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return self.n


def test_same_tensor_same_version_hits():
    m, build, t = Memo(), Counter(), torch.randn(5)
    assert m.get("s", (tkey(t), 7), build) == 1
    assert m.get("s", (tkey(t), 7), build) == 1 and build.n == 1
    assert m.peek("s") == 1


def test_an_in_place_write_misses():
    m, build, t = Memo(), Counter(), torch.randn(5)
    m.get("s", tkey(t), build)
    t.add_(1.0)
    assert m.get("s", tkey(t), build) == 2
    t[0] = 3.0
    assert m.get("s", tkey(t), build) == 3


def test_an_equal_valued_other_tensor_misses():
    m, build, t = Memo(), Counter(), torch.randn(5)
    m.get("s", tkey(t), build)
    assert m.get("s", tkey(t.clone()), build) == 2
    assert m.get("s", tkey(t.view(5)), build) == 3  # another tensor object over the same storage
    assert tkey(t) != tkey(t.view(1, 5)) and tkey(t) == tkey(t)


def test_a_key_of_several_tensors_follows_each_of_them():
    a, b = torch.randn(3), torch.randn(3)
    k = tkey(a, b)
    assert k == tkey(a, b) and k != tkey(b, a) and k != tkey(a) and k != tkey(a, b.clone())
    b.mul_(2.0)
    assert k != tkey(a, b)


def test_an_entry_keeps_its_source_tensor_alive():
    """The key holds the tensor (and its storage), so no other tensor can be handed its address while the entry lives."""
    m, t = Memo(), torch.randn(1000)
    ref = weakref.ref(t)
    m.get("s", tkey(t), lambda: 1)
    del t
    gc.collect()
    assert ref() is not None
    m.clear("s")
    gc.collect()
    assert ref() is None


def test_a_changed_plain_part_or_frame_token_misses():
    m, build, t = Memo(), Counter(), torch.randn(5)
    m.get("s", (tkey(t), "cuda:0", None), build)
    assert m.get("s", (tkey(t), "cuda:0", None), build) == 1
    assert m.get("s", (tkey(t), "cuda:1", None), build) == 2
    assert m.get("s", (tkey(t), "cuda:1", 1), build) == 3   # a frame token: the caller rewrote t through a raw pointer
    assert m.get("s", (tkey(t), "cuda:1", 2), build) == 4
    assert m.get("s", (tkey(t), "cuda:1", 2), build) == 4


def test_a_raising_build_stores_nothing():
    m, t = Memo(), torch.randn(5)
    m.get("s", 1, lambda: "old")

    def fail():
        raise RuntimeError("capture failed")

    with pytest.raises(RuntimeError, match="capture failed"):
        m.get("s", tkey(t), fail)
    assert m.peek("s") == "old" and m.get("s", 1) == "old"
    assert m.get("s", tkey(t)) is None  # (no build: a lookup)
    assert m.peek("s") == "old"


def test_a_slot_keeps_its_last_n_entries_most_recently_used_last():
    m = Memo(lru=3)
    for k in "abc":
        m.get("lru", k, lambda k=k: k.upper())
    assert m.get("lru", "a") == "A"  # a becomes the most recent one: b is the oldest now
    m.get("lru", "d", lambda: "D")
    assert m.get("lru", "b") is None
    assert [m.get("lru", k) for k in "acd"] == ["A", "C", "D"]
    m.get("lru", "e", lambda: "E")  # evicts a
    assert m.get("lru", "a") is None and m.peek("lru") == "E"
    m.get("one", 1, lambda: 1)  # slots are independent, size 1 unless given
    m.get("one", 2, lambda: 2)
    assert m.get("one", 1) is None and m.get("lru", "c") == "C"
    m.clear()
    assert m.peek("lru") is None and m.peek("one") is None


def _stub_device_packing(monkeypatch):
    marker = torch.arange(-31000, -30936, dtype=torch.int16)  # 64 values no parameter of a fresh Network holds as bytes

    monkeypatch.setattr(ops, "enc_conv_pack16", lambda w, backward_input=False: marker.clone())
    monkeypatch.setattr(ops, "make_pose", lambda R, Th, bounds, device=None: torch.zeros(15))
    return marker.numpy().tobytes()


def test_copies_and_pickles_carry_empty_memos(monkeypatch):
    marker = _stub_device_packing(monkeypatch)
    net = Network(num_train_frame=3)
    conv = net.xyzc_net.conv2[0]
    packed = net.xyzc_net._packed16(conv)
    assert net.xyzc_net._packed16(conv) is packed  # kept per (conv, weight)
    R, Th, bounds = torch.eye(3)[None], torch.zeros(1, 1, 3), torch.zeros(1, 2, 3)
    pose = net._pose_block(R, Th, bounds, torch.device("cpu"), None)
    assert net._memo.peek("pose") is pose
    r = Renderer(net, RenderConfig(N_samples=8, H=8, W=8))
    assert r._host_out_sh(torch.tensor([[8, 8, 8]], dtype=torch.int32)) == [8, 8, 8]
    r._tile_order({"mask_at_box": torch.ones(1, 64, dtype=torch.bool)}, 64, 0, 64)
    assert r._memo.peek("out_sh") is not None and r._memo.peek("order_full") is not None

    blob = pickle.dumps(net)
    assert marker not in blob  # the packed conv forms are not pickled (they were module attributes once)
    for net2, r2 in [(copy.deepcopy(net), copy.deepcopy(r)), (pickle.loads(blob), pickle.loads(pickle.dumps(r)))]:
        assert net2.xyzc_net._memo.peek((net2.xyzc_net.conv2[0], False)) is None and net2._memo.peek("pose") is None
        assert r2._memo.peek("out_sh") is None and r2._memo.peek("order_full") is None and r2.net._memo.peek("pose") is None
        assert torch.equal(net2.fc_0.weight, net.fc_0.weight)
        # ... and the copies' memos work, with the sizes of the originals
        assert net2.xyzc_net._packed16(net2.xyzc_net.conv2[0]) is not packed
        for b in range(9):
            r2._tile_order({"mask_at_box": torch.ones(1, 64, dtype=torch.bool)}, 64, 0, 64 - b)
        assert len(r2._memo._slots["order_full"]) == 8
    assert net._memo.peek("pose") is pose and net.xyzc_net._packed16(conv) is packed  # the originals keep theirs
