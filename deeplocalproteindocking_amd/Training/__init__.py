from .LocalTrainer import LocalTrainer
