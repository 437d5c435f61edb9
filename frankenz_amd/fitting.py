"""Import path used by the reference's demos (frankenz/fitting.py:25-30):
``from frankenz.fitting import BruteForce, NearestNeighbors, SelfOrganizingMap, GrowingNeuralGas``."""
from .bruteforce import BruteForce
from .knn import NearestNeighbors
from .networks import SelfOrganizingMap, GrowingNeuralGas

__all__ = ["BruteForce", "NearestNeighbors", "SelfOrganizingMap", "GrowingNeuralGas"]
