from .DockerParser import DockerParser, kabsch_rmsd
from . import InterfaceSelection
from .InterfaceSelection import evaluate_target, evaluate_target_device, native_reference
