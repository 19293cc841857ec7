"""zhusuan/_binding.py, the one loaded-library class and marshalling helpers behind the four ctypes bindings, on the host: the
C oracle's shared object (the main library's ABI built for the CPU) stands in for a kernel library, and ``flat_table`` only
takes addresses, so CPU tensors do.  No device library is needed."""
import ctypes

import pytest
import torch

import conftest
from zhusuan import _binding, _flow_hip, _hip, _hmc_hip, _mcmc_hip

_p, _i64, _u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64
PHILOX = {"zs_philox_normal_f32": [_p, _i64, _u64, _u64, _p, _p]}
WHO = {"zhusuan.mcmc": (_mcmc_hip.McmcTensor, None), "zhusuan.mcmc.HMC": (_hmc_hip.HmcTensor, 2)}


def oracle(**kw):
    args = dict(who="zhusuan.test", make_target="test", abi_symbol="zs_abi_version", abi_version=_hip.ABI_VERSION,
                prototypes=PHILOX)
    args.update(kw)
    return _binding.Library(conftest.build_oracle_lib(), **args)


def test_library_binds_calls_and_reports_errors():
    k = oracle(prototypes=dict(PHILOX, zs_build_info=(ctypes.c_char_p, [])))
    assert k.path == conftest.build_oracle_lib() and k.cdll.zs_abi_version() == _hip.ABI_VERSION
    assert isinstance(k.raw("zs_build_info"), bytes)                       # a (restype, argtypes) prototype
    out = torch.zeros(8, dtype=torch.float32)
    k.call("zs_philox_normal_f32", out.data_ptr(), 8, 1, 2, None, None)    # argtypes alone: an int return code, 0 = ok
    assert bool((out != 0).all())
    assert k.raw("zs_philox_normal_f32", None, 8, 1, 2, None, None) == -1
    with pytest.raises(RuntimeError, match=r"zs_philox_normal_f32 failed with code -1: invalid argument \(ZS_EINVAL\)"):
        k.call("zs_philox_normal_f32", None, 8, 1, 2, None, None)
    with pytest.raises(RuntimeError, match="zs_philox_normal_f32 failed with code -1: mine"):
        oracle(errors={-1: "mine"}).call("zs_philox_normal_f32", None, 8, 1, 2, None, None)


def test_abi_mismatch_names_both_versions():
    with pytest.raises(RuntimeError, match=r"zhusuan\.test: .*libzs_oracle.* has ABI version %d, expected %d"
                       % (_hip.ABI_VERSION, _hip.ABI_VERSION + 1)):
        oracle(abi_version=_hip.ABI_VERSION + 1)


def test_missing_symbol_is_an_attribute_error():
    with pytest.raises(AttributeError):
        oracle(prototypes=dict(PHILOX, zs_no_such_entry_f32=[_p]))


def test_missing_file_names_the_make_target(tmp_path):
    path = str(tmp_path / "libzs_none.so")
    with pytest.raises(RuntimeError) as e:
        _binding.Library(path, who="zhusuan.test", what="test library", make_target="test", abi_symbol="zs_abi_version",
                         abi_version=1, prototypes={})
    assert str(e.value) == ("zhusuan.test (MI355X build): test library not found at %s -- run `make -C zhusuan-pytorch_amd/csrc "
                            "test` (or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback." % path)
    for module, head, target in ((_mcmc_hip, "zhusuan.mcmc (MI355X build): sampler kernel library", "mcmc"),
                                 (_flow_hip, "zhusuan.invertible (MI355X build): flow kernel library", "flow"),
                                 (_hmc_hip, "zhusuan.mcmc.HMC (MI355X build): kernel library", "hmc")):
        with pytest.raises(RuntimeError) as e:
            module.lib(path)
        assert str(e.value).startswith(head + " not found at %s -- run `make -C zhusuan-pytorch_amd/csrc %s` " % (path, target))
        assert str(e.value).endswith("There is no CPU fallback.")
    with pytest.raises(RuntimeError, match=r"zhusuan \(MI355X build\): kernel library not found at .* \(or `make -C "
                                           r"zhusuan-pytorch_amd/csrc`\)\. There is no CPU fallback\."):
        _hip.KernelLibrary(path)


def test_lib_with_a_path_is_fresh_and_leaves_the_cache_alone():
    module = {"_LIB": None, "LIB_PATH": conftest.build_oracle_lib()}
    loaded = []

    def load(path):
        loaded.append(path)
        return oracle()

    cached = _binding.lazy_lib(module, load)
    assert module["_LIB"] is cached and _binding.lazy_lib(module, load) is cached and loaded == [module["LIB_PATH"]]
    fresh = _binding.lazy_lib(module, load, "elsewhere.so")
    assert fresh is not cached and module["_LIB"] is cached and loaded[1:] == ["elsewhere.so"]
    assert _binding.lazy_lib(module, load) is cached and len(loaded) == 2


@pytest.mark.parametrize("module,loader", [(_mcmc_hip, "McmcLibrary"), (_hmc_hip, "HmcLibrary"), (_flow_hip, "FlowLibrary")])
def test_a_satellites_lib_follows_the_same_contract(monkeypatch, module, loader):
    loaded = []

    def load(path):
        loaded.append(path)
        return object()

    monkeypatch.setattr(module, loader, load)
    monkeypatch.setattr(module, "_LIB", None)
    cached = module.lib()
    assert module._LIB is cached and module.lib() is cached and loaded == [module.LIB_PATH]
    fresh = module.lib("elsewhere.so")
    assert fresh is not cached and module._LIB is cached and module.lib() is cached and loaded[1:] == ["elsewhere.so"]


def test_suffix_and_u64():
    assert _binding.suffix(torch.float32, "%s") == "_f32" and _binding.suffix(torch.float64, "%s") == "_f64"
    with pytest.raises(RuntimeError, match="my words: torch.float16"):
        _binding.suffix(torch.float16, "my words: %s")
    assert _binding.u64(-1) == 2 ** 64 - 1 and _binding.u64(2 ** 64 + 5) == 5 and _binding.u64(7) == 7
    assert _binding.both({"f": [_p]}) == {"f_f32": [_p], "f_f64": [_p]}


def test_flat_table_of_two_tensors():
    a, b = torch.zeros(3, 2), torch.zeros(5)
    ga, sb = torch.ones(6), torch.ones(5)
    table, n, every = _binding.flat_table(_mcmc_hip.McmcTensor, dict(q_in=[a, b], q_out=[a, b], grad=[ga, None], state=[None, sb],
                                                                     z=None), [a, b], "zhusuan.mcmc")
    assert len(table) == 2 and n == 11 and [t.start for t in table] == [0, 6]
    assert [(t.q_in, t.q_out, t.grad, t.state, t.z) for t in table] == [(a.data_ptr(), a.data_ptr(), ga.data_ptr(), None, None),
                                                                        (b.data_ptr(), b.data_ptr(), None, sb.data_ptr(), None)]
    assert [id(t) for t in every] == [id(t) for t in (a, a, ga, b, b, sb)]
    empty, n0, every0 = _binding.flat_table(_mcmc_hip.McmcTensor, dict(q_in=[]), [], "zhusuan.mcmc")
    assert len(empty) == 1 and n0 == 0 and every0 == []


def test_flat_table_of_three_tensors_with_chains():
    C = 2
    q = [torch.zeros(C, 3), torch.zeros(C, 1, dtype=torch.float32), torch.zeros(C, 4, 5)]
    p = [torch.ones_like(t) for t in q]
    z = [None, torch.ones(C), None]
    table, n, every = _binding.flat_table(_hmc_hip.HmcTensor, dict(q0=None, q=q, p=p, z=z), q, "zhusuan.mcmc.HMC", C)
    assert n == 6 + 2 + 40 and [t.start for t in table] == [0, 6, 8] and [t.row for t in table] == [3, 1, 20]
    assert [t.q for t in table] == [t.data_ptr() for t in q] and [t.p for t in table] == [t.data_ptr() for t in p]
    assert [t.z for t in table] == [None, z[1].data_ptr(), None]
    assert all(t.q0 is None and t.grad is None and t.p0 is None and t.q_out is None for t in table)
    assert len(every) == 7


@pytest.mark.parametrize("who", sorted(WHO))
def test_flat_table_rejects_what_the_kernels_cannot_read(who):
    struct, n_chains = WHO[who]
    field = struct._fields_[0][0]
    a, b = torch.zeros(2, 4), torch.zeros(2, 3)
    message = "^%s: operands of one latent must be contiguous, of one dtype and one size$" % who.replace(".", r"\.")
    for bad in (torch.zeros(4, 2).t(),                        # not contiguous
                torch.zeros(2, 4, dtype=torch.float64),       # a second dtype
                torch.zeros(2, 5)):                           # another size
        with pytest.raises(RuntimeError, match=message):
            _binding.flat_table(struct, {field: [a, b], "grad": [bad, None]}, [a, b], who, n_chains)
    with pytest.raises(RuntimeError, match=message):          # one dtype over the whole table, the first tensor's
        _binding.flat_table(struct, {field: [a, b.double()]}, [a, b.double()], who, n_chains)
