#!/usr/bin/env python3
"""How the REFERENCE's own build_tacotron (tacotron/tacotron.py:165-224) assembles the LJSpeech model
(configs/config-ljspeech.yaml): the constructor calls it makes and the state-dict keys / shapes of what it builds.
tests/test_host_logic.py replays those calls on the drop-in classes without the reference.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_integration.py <torch-tts checkout>
Writes tests/golden/integration_ljspeech.json (config values, call arguments, key names and shapes; no reference source)."""
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
import yaml  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]
sys.path.insert(0, os.path.join(REF, "tacotron"))
import tacotron as ref_tacotron  # noqa: E402

# the classes build_tacotron instantiates for this config; a module passed as an argument is recorded as "<ClassName>"
CLASSES = ("Taco2ProdDecoderCell", "Decoder", "Encoder2", "MelPostnet", "Tacotron")


def main():
    cfg = yaml.safe_load(open(os.path.join(REF, "configs", "config-ljspeech.yaml")))
    calls = []

    def value(a):
        return f"<{type(a).__name__}>" if hasattr(a, "state_dict") else a

    def recording(cls):
        class Rec(cls):
            def __init__(self, *args, **kwargs):
                calls.append({"class": cls.__name__, "args": [value(a) for a in args], "kwargs": {k: value(v) for k, v in kwargs.items()}})
                super().__init__(*args, **kwargs)

        Rec.__name__ = cls.__name__
        return Rec

    for name in CLASSES:
        setattr(ref_tacotron, name, recording(getattr(ref_tacotron, name)))
    model = ref_tacotron.build_tacotron(cfg)
    out = {
        "reference": "kgoba/torch-tts @ 2024_10_08, tacotron/tacotron.py build_tacotron on configs/config-ljspeech.yaml",
        "config": {"text": {"alphabet": cfg["text"]["alphabet"]}, "audio": cfg["audio"], "model": cfg["model"]},
        "calls": calls,
        "state_dict": {k: list(v.shape) for k, v in model.state_dict().items()},
    }
    with open(os.path.join(HERE, "integration_ljspeech.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(len(calls), "calls,", len(out["state_dict"]), "state-dict keys")


if __name__ == "__main__":
    main()
