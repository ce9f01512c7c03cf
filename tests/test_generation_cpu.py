"""No GPU: the KV cache and the decoding code are modules of their own -- importable without the model classes -- and every name that
moved there is still the same object through `modeling_core`."""
import os
import subprocess
import sys

from helpers import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOVED = {
    "kv_cache": ("KVCache", "KV_CACHE_DTYPES", "_check_kv_dtype"),
    "generation": ("GenerateOutput", "no_repeat_ngram_banned_tokens", "prompt_lookup_candidates", "check_prompt_lookup", "sampling_probs",
                   "check_sampler"),
}


def test_generation_and_kv_cache_import_without_the_model():
    code = ("import importlib, sys\n"
            "importlib.import_module('u-llava_amd.generation'); importlib.import_module('u-llava_amd.kv_cache')\n"
            "assert 'u-llava_amd.modeling_core' not in sys.modules and 'u-llava_amd.modeling_ullava' not in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_moved_names_are_the_same_objects_through_modeling_core():
    MC = pkg("modeling_core")
    for mod, names in MOVED.items():
        for name in names:
            assert getattr(MC, name) is getattr(pkg(mod), name), (mod, name)
    assert pkg("kv_cache").DEFAULT_HEADROOM == 512
    for gone in ("_cache_headroom", "_new_cache_kv_dtype", "_kv8_attention", "_kv8_decode_buffers", "_generate_prompt_lookup"):
        assert not hasattr(MC.UllavaCoreForCausalLM, gone), gone
