"""Input pipeline of the training harness: LIDC preparation + mini-batch provider, with the batch assembly and
augmentation running on the GPU over an HBM-resident dataset (data/batch_provider.py, data/lidc_data_loader.py, data/lidc_data.py
of the reference), and the BraTS volume dataset of the 3-D model on the same terms (data/bratsDataset.py,
data/BratsProcessing/augmentation.py), with raw cases in and native-space maps out (data/BratsProcessing/brats18_data_loader.py,
brats18_validation_data_loader.py)."""
from .batch_provider import BatchProvider  # noqa: F401
from .lidc_data import lidc_data  # noqa: F401
from .brats_dataset import BratsDataset  # noqa: F401
from .brats_prepare import PreparedCase, PreparedSplit, prepare_case, prepare_cases, restore_volume  # noqa: F401
